"""Static check of the merged-launch protocol (csrc/asm_bt.hip.h, csrc/asm_batch.hip.h) over every kernel of the library.

Every __global__ definition has two ways of receiving its arguments: as kernel arguments (bt.tab == nullptr), or - in a merged launch of a
scenario batch - from an argument table in HBM that the host packs in declaration order (asmb::pk_write) and ASM_BARGS unpacks in the order
of ITS list.  A list that misses a parameter or names them in another order compiles and passes every per-handle test, so this file reads
the sources and asserts, for every kernel:
  * the first parameter is an AsmBt, and the first statement of the body is ASM_BARGS(<that parameter>, <every other parameter, in
    declaration order>) - only #pragma lines may precede it;
and for the sources as a whole:
  * blockIdx.z / gridDim.z only in asm_bt.hip.h (kernels read asm_bz), <<< only in asm_batch.hip.h (everything launches through the
    recorder), no other launch API, no dynamic LDS (the recorder passes 0 bytes);
  * no __device__ / __constant__ / __managed__ variable: the scenarios of one merged launch would share it.
The number of kernels checked must equal the number of __global__ tokens in code, so a definition the parser cannot read fails the test.
Code inside #ifdef blocks of macros that the sources never define (the diagnostic builds) is not part of the library and is skipped.
The negative controls feed the same checker small sources with one defect each."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "activesetmethods_amd", "csrc")
BT_HEADER, RECORDER = "asm_bt.hip.h", "asm_batch.hip.h"
NOT_COMPILED = []          # "file:line name" of kernels inside #ifdef blocks of the diagnostic builds: none today


def strip_comments(src):
    """Comments replaced by blanks (newlines kept, so #-directives stay line-bound); string and character literals are left alone."""
    out, i, n = [], 0, len(src)
    while i < n:
        c = src[i]
        if c == '"' or c == "'":
            j = i + 1
            while j < n and src[j] != c:
                j += 2 if src[j] == "\\" else 1
            out.append(src[i:j + 1])
            i = j + 1
        elif src.startswith("//", i):
            j = src.find("\n", i)
            j = n if j < 0 else j
            while j < n and src[j - 1] == "\\":          # a continued // comment
                j = src.find("\n", j + 1)
                j = n if j < 0 else j
            i = j
        elif src.startswith("/*", i):
            j = src.find("*/", i + 2)
            j = n if j < 0 else j + 2
            out.append("\n" * src.count("\n", i, j) + " ")
            i = j
        else:
            out.append(c)
            i += 1
    return "".join(out)


def defined_macros(sources):
    return set(m for s in sources.values() for m in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)", s, flags=re.M))


def drop_inactive(src, macros):
    """Lines inside #ifdef X / #ifndef X blocks that the default build does not compile become empty.  An #ifndef X whose first line is
    #define X is live (an include guard, or the default of a macro the command line may set).  Other conditionals (#if) keep every branch."""
    out, stack = [], []                 # stack entries: [active, known]
    lines = src.split("\n")
    for i, line in enumerate(lines):
        m = re.match(r"[ \t]*#[ \t]*(ifdef|ifndef|if|elif|else|endif)\b[ \t]*(\w*)", line)
        kind = m.group(1) if m else None
        if kind in ("ifdef", "ifndef"):
            nxt = next((l for l in lines[i + 1:] if l.strip()), "")
            own = kind == "ifndef" and re.match(r"[ \t]*#[ \t]*define[ \t]+%s\b" % re.escape(m.group(2)), nxt)
            stack.append([bool(own) or (m.group(2) in macros) == (kind == "ifdef"), True])
        elif kind == "if":
            stack.append([True, False])
        elif kind == "elif" and stack:
            stack[-1] = [True, False]
        elif kind == "else" and stack:
            if stack[-1][1]:
                stack[-1][0] = not stack[-1][0]
        elif kind == "endif" and stack:
            stack.pop()
        elif all(a for a, _ in stack):
            out.append(line)
            continue
        out.append("")
    return "\n".join(out)


def kernel_names(sources):
    """(names of the __global__ functions in the code the default build compiles, "file:line name" of those in blocks it does not)."""
    clean = {k: strip_comments(v) for k, v in sources.items()}
    macros = defined_macros(clean)
    live, skipped = [], []
    for name in sorted(clean):
        kept = drop_inactive(clean[name], macros).split("\n")
        for m in re.finditer(r"\b__global__\b", clean[name]):
            line = clean[name].count("\n", 0, m.start())
            k = re.search(r"\bvoid\s+(\w+)\s*\(", clean[name][m.end():m.end() + 400])
            kn = k.group(1) if k else "?"
            if "__global__" in kept[line]:
                live.append(kn)
            else:
                skipped.append("%s:%d %s" % (name, line + 1, kn))
    return live, skipped


def _close(src, i, op, cl):
    """index just past the bracket that closes the one opening at src[i]"""
    depth = 0
    for j in range(i, len(src)):
        if src[j] == op:
            depth += 1
        elif src[j] == cl:
            depth -= 1
            if depth == 0:
                return j + 1
    return -1


def _split_top(s):
    parts, depth, cur = [], 0, []
    for ch in s:
        if ch in "(<[{":
            depth += 1
        elif ch in ")>]}":
            depth -= 1
        if ch == "," and depth == 0:
            parts.append("".join(cur))
            cur = []
        else:
            cur.append(ch)
    if "".join(cur).strip():
        parts.append("".join(cur))
    return [p.strip() for p in parts]


def _param_name(p):
    p = re.sub(r"\[[^\]]*\]\s*$", "", p.split("=")[0].strip())
    m = re.search(r"(\w+)\s*$", p)
    return m.group(1) if m else None


def check_kernels(name, src, problems):
    """every __global__ token of `src` (comments stripped): a definition that follows the protocol.  Returns (tokens, kernels checked)."""
    tokens = checked = 0
    for m in re.finditer(r"\b__global__\b", src):
        tokens += 1
        where = "%s:%d" % (name, src.count("\n", 0, m.start()) + 1)
        i = m.end()
        while True:                     # __launch_bounds__(...) and __attribute__((...)), in any order and number
            a = re.compile(r"\s*(__launch_bounds__|__attribute__)\s*\(").match(src, i)
            if not a:
                break
            i = _close(src, a.end() - 1, "(", ")")
        h = re.compile(r"\s*(?:static\s+|inline\s+)*void\s+(\w+)\s*\(").match(src, i)
        if not h or i < 0:
            problems.append("%s: a __global__ the parser cannot read" % where)
            continue
        kname, end = h.group(1), _close(src, h.end() - 1, "(", ")")
        params = _split_top(src[h.end():end - 1])
        b = re.compile(r"\s*\{").match(src, end)
        if not b:
            problems.append("%s: %s is not a definition" % (where, kname))
            continue
        checked += 1
        if not params or not re.match(r"(const\s+)?AsmBt\b(?!\s*[*&])", params[0]):
            problems.append("%s: %s: the first parameter is not an AsmBt" % (where, kname))
            continue
        names = [_param_name(p) for p in params]
        body = re.sub(r"^[ \t]*#[ \t]*pragma[^\n]*$", "", src[b.end():b.end() + 4000], flags=re.M)
        s = re.match(r"\s*ASM_BARGS\s*\(([^()]*)\)\s*;", body)
        if not s:
            problems.append("%s: %s: the body does not start with ASM_BARGS(...)" % (where, kname))
            continue
        listed = [a.strip() for a in s.group(1).split(",")]
        if listed != names:
            missing, extra = [x for x in names if x not in listed], [x for x in listed if x not in names]
            what = ("missing %s" % missing if missing else "") + (" extra %s" % extra if extra else "")
            problems.append("%s: %s: ASM_BARGS list %s does not match the parameters %s (%s)" % (where, kname, listed, names, what.strip() or "order"))
    return tokens, checked


def check_sources(sources):
    """sources: {file name: text}.  Returns (tokens, kernels checked, problems)."""
    clean = {k: strip_comments(v) for k, v in sources.items()}
    macros = defined_macros(clean)
    clean = {k: drop_inactive(v, macros) for k, v in clean.items()}
    problems, tokens, checked = [], 0, 0
    for name in sorted(clean):
        src = clean[name]
        t, c = check_kernels(name, src, problems)
        tokens, checked = tokens + t, checked + c

        def report(pattern, what, src=src, name=name):
            for m in re.finditer(pattern, src):
                problems.append("%s:%d: %s" % (name, src.count("\n", 0, m.start()) + 1, what))
        if name != BT_HEADER:
            report(r"\b(blockIdx|gridDim)\s*\.\s*z\b", "blockIdx.z / gridDim.z outside %s (kernels read asm_bz)" % BT_HEADER)
        if name != RECORDER:
            report(r"<<<", "a <<< launch outside %s" % RECORDER)
        report(r"\bhipLaunchKernelGGL\b|\bhipModuleLaunchKernel\b|\bhipLaunchCooperativeKernel\w*|\bhipExtLaunch\w*|\bhipLaunchKernel\b",
               "a launch that does not go through the recorder")
        report(r"\bextern\s+__shared__\b", "dynamic LDS (the recorder passes 0 bytes)")
        report(r"\b(__constant__|__managed__)\b", "a __constant__ / __managed__ variable: shared by the scenarios of one launch")
        for m in re.finditer(r"\b__device__\b", src):
            decl = re.sub(r"__attribute__\s*\(\(.*?\)\)|alignas\s*\([^)]*\)", " ", re.split(r"[;{=]", src[m.end():m.end() + 2000], 1)[0])
            if "(" not in decl:
                problems.append("%s:%d: a __device__ variable: shared by the scenarios of one launch" % (name, src.count("\n", 0, m.start()) + 1))
    return tokens, checked, problems


def _library_sources():
    files = sorted(set(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hip.h"))))
    return {os.path.basename(f): open(f).read() for f in files}


def test_every_kernel_follows_the_merged_launch_protocol():
    src = _library_sources()
    assert BT_HEADER in src and RECORDER in src and "asm_hip.hip" in src
    tokens, checked, problems = check_sources(src)
    live, skipped = kernel_names(src)
    print("kernels checked: %d of %d __global__ tokens in code; in blocks the default build does not compile: %s" % (checked, tokens, skipped or "none"))
    assert not problems, "\n".join(problems)
    assert checked == tokens and checked > 200, (checked, tokens)
    # every __global__ token of the sources is a kernel that was checked or one named here: nothing leaves the check unseen
    assert len(live) == checked and skipped == NOT_COMPILED, (len(live), checked, skipped)


GOOD = """
// a comment that says __global__ and blockIdx.z and <<<
template <int T>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
void k_good(AsmBt abt, const double* __restrict__ A, int64_t ld, Pack<T, 2> P, unsigned* __restrict__ flags, int n) {
#pragma clang fp contract(off)
    ASM_BARGS(abt, A, ld, P, flags, n);
    A[asm_bz(abt)] = 0;
}
__device__ __forceinline__ double helper(double a, double b = 1.0) { return a * b; }
#ifdef NEVER_DEFINED_PROF
__device__ unsigned long long g_prof[8];
#endif
"""


def _problems(text, name="x.hip.h"):
    tokens, checked, problems = check_sources({name: text})
    return tokens, checked, problems


def test_the_checker_accepts_a_correct_kernel():
    tokens, checked, problems = _problems(GOOD)
    assert (tokens, checked, problems) == (1, 1, [])


def test_negative_controls():
    def one(text, needle, name="x.hip.h"):
        problems = _problems(text, name)[2]
        assert len(problems) >= 1 and any(needle in p for p in problems), (needle, problems)
    k = "__global__ __launch_bounds__(64) void k(AsmBt bt, double* a, int n, double s) {\n    %s\n}\n"
    assert _problems(k % "ASM_BARGS(bt, a, n, s);")[2] == []
    one(k % "ASM_BARGS(bt, a, s, n);", "(order)")                                            # reordered
    one(k % "ASM_BARGS(bt, a, n);", "missing ['s']")                                         # a name missing
    one(k % "ASM_BARGS(bt, a, n, s, t);", "extra ['t']")                                     # a name too many
    one(k % "ASM_BARGS(abt, a, n, s);", "does not match")                                    # another table
    one(k % "int i = 0; ASM_BARGS(bt, a, n, s);", "does not start with ASM_BARGS")           # a statement before it
    one(k % "a[0] = s;", "does not start with ASM_BARGS")                                    # no prologue
    one("__global__ void k(double* a, AsmBt bt) {\n    ASM_BARGS(bt, a);\n}\n", "first parameter is not an AsmBt")
    one("__global__ void k(AsmBt bt, double* a);\n", "not a definition")
    one(k % "ASM_BARGS(bt, a, n, s); a[blockIdx.z] = s;", "blockIdx.z")                      # raw blockIdx.z
    one(k % "ASM_BARGS(bt, a, n, s); a[gridDim . z] = s;", "blockIdx.z")
    assert _problems(k % "ASM_BARGS(bt, a, n, s); a[blockIdx.z] = s;", BT_HEADER)[2] == []
    launch = "void f(double* a) { k<<<dim3(1), dim3(64), 0, nullptr>>>(AsmBt{nullptr, 0, 1}, a, 1, 0.0); }\n"
    one(launch, "<<<")
    assert _problems(launch, RECORDER)[2] == []
    one("void f() { hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, 0, 1); }\n", "does not go through the recorder")
    one("void f() { hipModuleLaunchKernel(fn, 1, 1, 1, 64, 1, 1, 0, 0, args, 0); }\n", "does not go through the recorder")
    one("void f() { hipLaunchCooperativeKernel(k, g, b, args, 0, 0); }\n", "does not go through the recorder")
    one(k % "ASM_BARGS(bt, a, n, s); extern __shared__ double sm[];", "dynamic LDS")
    one("__device__ unsigned g_count;\n", "__device__ variable")
    one("__device__ double g_tab[4] = {0, 1, 2, 3};\n", "__device__ variable")
    one("__constant__ double c_tab[4];\n", "__constant__")
    one("__managed__ int g_flag;\n", "__managed__")
    # a kernel the parser cannot read is counted as a token and not as a kernel: the count check of the library test fails
    tokens, checked, problems = _problems("__global__ int k(AsmBt bt) { }\n")
    assert tokens == 1 and checked == 0 and problems


def test_comments_strings_and_inactive_blocks_are_not_code():
    assert "blockIdx" not in strip_comments("a /* blockIdx.z */ b // blockIdx.z\n")
    assert strip_comments('s = "// not a comment";') == 's = "// not a comment";'
    src = "#define ON 1\n#ifdef ON\nint a;\n#else\nint b;\n#endif\n#ifndef OFF\nint c;\n#endif\n#ifdef OFF\nint d;\n#endif\n"
    kept = drop_inactive(src, defined_macros({"x": src}))
    assert "int a;" in kept and "int c;" in kept and "int b;" not in kept and "int d;" not in kept
    assert kept.count("\n") == src.count("\n")
    guard = "#ifndef X_H\n#define X_H\n__global__ void k(AsmBt bt) {\n    ASM_BARGS(bt);\n}\n#endif\n#ifdef PROF\n__global__ void k_prof(AsmBt bt) {\n}\n#endif\n"
    assert "__global__" in drop_inactive(guard, defined_macros({"x": guard}))          # an include guard hides nothing
    assert kernel_names({"x.hip.h": guard}) == (["k"], ["x.hip.h:8 k_prof"])
