"""CPU checks of the entries that run the kernel hooks on the fibers of a scenario batch (include/asm_hip.h: asm_batch_test_run,
asm_batch_test_record_size, asm_test_copy_fill, asm_test_batch_kernel_counting, asm_test_batch_kernel_table, asm_test_batch_panel_share): the header declares them, the
built library exports them, the ctypes binding covers them with the declared argument types, and every family's record - the hook's
parameters after h - has in the binding the size the library compiled."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("asm_test_copy_fill", "asm_batch_test_run", "asm_batch_test_record_size", "asm_test_batch_kernel_counting", "asm_test_batch_kernel_table",
       "asm_test_batch_panel_share")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "asm_hip.h")).read(), flags=re.S)


def test_header_declares_the_entries_the_library_exports_them_and_the_binding_covers_them():
    from activesetmethods_amd import _lib
    txt = _header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint(64_t)?\s+%s\s*\(" % name, txt), name
        assert hasattr(lib, name), "libasmhip.so does not export %s" % name
        assert name in _lib.PROTOTYPES, name
    P, i64, i32, u8 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.POINTER(ctypes.c_uint8)
    assert _lib.PROTOTYPES["asm_test_copy_fill"] == (ctypes.c_int, [P, ctypes.c_uint32, i64, i64, i64, i64, i64, i32, u8, u8, u8, u8, u8, u8])
    assert _lib.PROTOTYPES["asm_batch_test_run"] == (ctypes.c_int, [P, i32, i64, P, ctypes.POINTER(i32)])
    assert _lib.PROTOTYPES["asm_batch_test_record_size"] == (i64, [i32])
    assert _lib.PROTOTYPES["asm_test_batch_kernel_counting"] == (ctypes.c_int, [P, ctypes.c_int])
    assert _lib.PROTOTYPES["asm_test_batch_panel_share"] == (ctypes.c_int, [P, ctypes.c_int])
    assert _lib.PROTOTYPES["asm_test_batch_kernel_table"] == (ctypes.c_int, [P, ctypes.POINTER(_lib.BatchKernelRow), i64, ctypes.POINTER(i64), ctypes.c_int])
    assert ctypes.sizeof(_lib.BatchKernelRow) == 256 + 8 + 8 + 4 + 4
    assert re.search(r"char\s+name\[256\];\s*int64_t\s+operations,\s*launches;\s*int32_t\s+nb_max,\s*gz;\s*}\s*asm_batch_kernel_row", txt)


def test_families_and_records_match_the_header_and_the_library():
    from activesetmethods_amd import _lib
    txt = _header()
    m = re.search(r"enum\s*{\s*(ASM_TF_\w+\s*=\s*0[^}]*)}", txt)
    names = [e.split("=")[0].strip() for e in m.group(1).split(",")]
    assert names[-1] == "ASM_TF_COUNT" and len(names) - 1 == len(_lib.TEST_FAMILIES)
    lib = _lib.load()
    for fam, hook in enumerate(_lib.TEST_FAMILIES):
        assert names[fam] == "ASM_TF_" + hook[len("asm_test_"):].upper(), (fam, hook)
        # the record of the header: as many fields as the hook has parameters after h, and the size the binding gives its structure
        body = re.search(r"typedef\s+struct\s*{([^}]*)}\s*%s_args\s*;" % hook, txt)
        assert body, hook
        fields = sum(len(decl.split(",")) for decl in body.group(1).split(";") if decl.strip())
        rec = _lib.hook_record(hook)
        assert fields == len(rec._fields_) == len(_lib.PROTOTYPES[hook][1]) - 1, hook
        assert lib.asm_batch_test_record_size(fam) == ctypes.sizeof(rec), hook
    assert lib.asm_batch_test_record_size(len(_lib.TEST_FAMILIES)) == -1 and lib.asm_batch_test_record_size(-1) == -1


def test_bad_arguments_are_refused_before_any_device_is_touched():
    from activesetmethods_amd import _lib
    lib = _lib.load()
    n = ctypes.c_int64(0)
    assert lib.asm_batch_test_run(None, 0, 1, None, None) != 0
    assert lib.asm_test_batch_kernel_counting(None, 1) != 0
    assert lib.asm_test_batch_panel_share(None, 0) == -1
    assert lib.asm_test_batch_kernel_table(None, None, 0, ctypes.byref(n), 0) != 0
    assert lib.asm_test_copy_fill(None, 0, 0, 0, 0, 0, 0, 0, None, None, None, None, None, None) != 0
