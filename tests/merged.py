"""Helpers of the merged-launch tests (tests/test_merged_launch_gpu.py, tests/test_copy_fill_gpu.py): running a kernel hook's calls again as the
scenarios of a batch (asm_batch_test_run), and reading the per-kernel merge table (asm_test_batch_kernel_table).

`Capture` stands in for the library inside the helpers of the stage tests (their Run / Call / _stages take the library as an argument): every
call of a hook that asm_batch_test_run knows is made on the plain handle as usual - that is the reference, the call the stage tests compare with
their float128 / exact twins - and remembered with the contents its arrays had before it.  `Scenario.record()` then builds the same call as
a batch record on fresh copies of those arrays; after the batch ran, `Scenario.compare()` wants every array byte for byte as the plain call left
its own."""
import ctypes as C
import numbers

import numpy as np

from activesetmethods_amd import _lib

ERR_HIP = -2


class Scenario:
    def __init__(self, hook, args, before, rc):
        self.hook, self.args, self.before, self.rc = hook, args, before, rc
        self.fresh = None

    def record(self):
        """The call as a record of the hook's family, its arrays replaced by copies of what they held before the plain call."""
        Rec = _lib.hook_record(self.hook)
        rec, copies = Rec(), {}
        self.fresh = []
        for i, (a, b) in enumerate(zip(self.args, self.before)):
            typ = Rec._fields_[i][1]
            arr = None
            if b is not None:
                arr = copies.setdefault(id(a._arr), b.copy())          # (an array passed twice stays one array)
                v = arr.ctypes.data_as(typ)
            elif a is None:
                v = None
            elif isinstance(a, numbers.Integral):
                v = int(a)
            elif isinstance(a, numbers.Real):
                v = float(a)
            else:
                v = C.cast(a, typ)                                     # a ctypes array of stage structures: read only, shared
            self.fresh.append(arr)
            if v is not None:
                setattr(rec, "a%d" % i, v)
        return rec

    def compare(self, status, tag):
        assert status == self.rc, (tag, "status", status, self.rc)
        for i, (a, arr) in enumerate(zip(self.args, self.fresh)):
            if arr is not None:
                ref = a._arr
                assert arr.shape == ref.shape and arr.dtype == ref.dtype
                if arr.tobytes() != ref.tobytes():
                    bad = np.flatnonzero(arr.reshape(-1).view(np.uint8) != ref.reshape(-1).view(np.uint8))
                    raise AssertionError("%s: argument %d of %s differs from the plain-handle call in %d bytes, the first at byte %d of %d"
                                         % (tag, i + 1, self.hook, bad.size, bad[0], arr.nbytes))


class Capture:
    """The library, with the calls of the batch-capable hooks remembered (`calls`) and asm_sublp_setup's arguments kept (`setup`)."""

    def __init__(self, lib):
        self._lib, self.calls, self.setup = lib, [], None

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name == "asm_sublp_setup":
            def setup(h, *args):
                self.setup = args
                return fn(h, *args)
            return setup
        if name not in _lib.TEST_FAMILIES:
            return fn

        def call(h, *args):
            before = [a._arr.copy() if hasattr(a, "_arr") else None for a in args]
            rc = fn(h, *args)
            self.calls.append(Scenario(name, args, before, rc))
            return rc
        return call

    def last(self):
        return self.calls[-1]


def make_batch(lib, slots, groups=1):
    b = C.c_void_p()
    assert lib.asm_batch_create(0, slots, C.byref(b)) == 0
    assert lib.asm_batch_set_groups(b, groups) == 0 and lib.asm_batch_groups(b) == groups
    assert lib.asm_test_batch_kernel_counting(b, 1) == 0
    return b


def kernel_table(lib, b, reset=True):
    """[(name, operations, launches, nb_max, gz)] since the last reset."""
    n = C.c_int64(0)
    assert lib.asm_test_batch_kernel_table(b, None, 0, C.byref(n), 0) == 0
    rows = (_lib.BatchKernelRow * max(n.value, 1))()
    assert lib.asm_test_batch_kernel_table(b, rows, n.value, C.byref(n), 1 if reset else 0) == 0, lib.asm_batch_last_error(b)
    return [(r.name.decode(), int(r.operations), int(r.launches), int(r.nb_max), int(r.gz)) for r in rows[:n.value]]


def run_batch(lib, b, scenarios, tag):
    """The scenarios (calls of one hook) as one asm_batch_test_run; every array and status compared with the plain-handle calls.  Returns the
    kernel table of the run."""
    hook = scenarios[0].hook
    assert all(s.hook == hook for s in scenarios)
    Rec = _lib.hook_record(hook)
    recs = (Rec * len(scenarios))(*[s.record() for s in scenarios])
    status = np.full(len(scenarios), -99, np.int32)
    kernel_table(lib, b)                                   # (what set-up calls recorded does not count)
    rc = lib.asm_batch_test_run(b, _lib.TEST_FAMILIES.index(hook), len(scenarios), C.cast(recs, C.c_void_p), _lib.i32ptr(status))
    stop_after_device_error(lib, b, rc, status, tag)
    assert rc == 0, lib.asm_batch_last_error(b)
    tab = kernel_table(lib, b)
    for k, s in enumerate(scenarios):
        s.compare(int(status[k]), "%s, scenario %d" % (tag, k))
    return tab


def stop_after_device_error(lib, b, rc, status, tag):
    """A failed round or a device error inside a scenario (ASM_ERR_HIP) leaves the device in an unknown state: nothing more is started on it,
    the session ends here."""
    if rc == ERR_HIP or (status == ERR_HIP).any():
        import pytest
        pytest.exit("%s: device error in a batch run (%s) - the session ends here" % (tag, lib.asm_batch_last_error(b)), returncode=3)


SEEN = set()           # kernel names seen in a merged launch (nb_max >= 2) by the tests of this session


def note_merged(tab):
    SEEN.update(name for name, _, _, nb, _ in tab if nb >= 2)


def short(name):
    """A mangled kernel name without its parameter list: k_trtri_level<512> stays apart from k_trtri_level<1024>."""
    import re
    m = re.match(r"_Z(\d+)", name)
    if not m:
        return name.split("(")[0]
    ln = int(m.group(1))
    base = name[m.end():m.end() + ln]
    t = re.match(r"I((?:Li\d+E)+)E", name[m.end() + ln:])
    return base + ("<%s>" % ",".join(re.findall(r"Li(\d+)E", t.group(1))) if t else "")


def coverage_report():
    """Lines of the coverage report: the distinct kernels seen in a merged launch so far against the kernels of the source (the list the
    protocol checker reads, tests/test_kernel_protocol_cpu.py), and the ones not reached."""
    from tests.test_kernel_protocol_cpu import _library_sources, kernel_names
    import re
    defined = set(kernel_names(_library_sources())[0])
    seen = set(re.sub(r"<.*", "", short(k)).replace("void ", "").strip() for k in SEEN)
    return ["kernels seen in a merged launch by this run: %d of %d in the source" % (len(seen & defined), len(defined)),
            "seen: %s" % " ".join(sorted(seen)), "not reached: %s" % " ".join(sorted(defined - seen))]
