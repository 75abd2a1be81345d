"""The copy and fill kernels of the stream recorder (csrc/asm_batch.hip.h: k_bcopy, k_bfill) through the hook asm_test_copy_fill.

Both kernels pick a 16-, 8- (copy only), 4- or 1-byte branch by the joint alignment of destination, source and byte count, and walk the range
in a grid-stride loop under a capped grid: at most 256 workgroups on the plain path (asmb::copy_async / fill_async outside a fiber: the ~60
device-to-device copies of an LP), at most 64 on the recorded path (inside a fiber: every copy and fill of a scenario batch, host-to-device
payloads through the round's blob, device-to-host results through the staging buffer).  Each case runs on a plain handle and as three scenarios
of a batch - the same byte count at three different offsets, so one merged launch takes different branches per scenario - and is compared
byte for byte with NumPy slicing over the whole buffers, the 64-byte margins on either side included (the ranges end exactly at the margin)."""
import ctypes as C
import itertools

import numpy as np
import pytest

from activesetmethods_amd import _lib
from tests import merged

pytestmark = pytest.mark.gpu
H2D, D2D, FILL, D2H = 1, 2, 4, 8
ALL = H2D | D2D | FILL | D2H
OFFSETS = (0, 1, 2, 4, 8, 12)
COUNTS = (1, 3, 4, 5, 8, 12, 16, 17, 24, 32, 4100)
LOOP_64, LOOP_256 = 64 * 256 * 16 + 16, 256 * 256 * 16 + 16      # more 16-byte steps than 64 x 256 / 256 x 256 threads
VALUES = (0, 0xAB, 0x1AB, -1)
U8 = C.POINTER(C.c_uint8)
HOST_FILL = 0x5A


@pytest.fixture(scope="module")
def handle(hip_lib):
    h = C.c_void_p()
    assert hip_lib.asm_create(0, C.byref(h)) == 0
    yield h
    hip_lib.asm_destroy(h)


@pytest.fixture(scope="module")
def batch(hip_lib):
    b = merged.make_batch(hip_lib, 3)
    yield b
    hip_lib.asm_batch_destroy(b)
    print("\nkernels seen in a merged launch: %s" % sorted(merged.short(k) for k in merged.SEEN))


class Case:
    """The arguments of one call and what NumPy makes of them."""

    def __init__(self, ops, nbytes, dst=0, src=0, fo=0, value=0, seed=0, span=None):
        rng = np.random.default_rng(seed)
        self.ops, self.nbytes, self.dst, self.src, self.fo, self.value = ops, nbytes, dst, src, fo, value
        self.span = nbytes + max(dst, src, fo) if span is None else span      # the furthest range ends at the margin
        total = 64 + self.span + 64
        self.a0, self.b0 = rng.integers(0, 256, total, dtype=np.uint8), rng.integers(0, 256, total, dtype=np.uint8)
        self.hsrc = rng.integers(0, 256, max(nbytes, 1), dtype=np.uint8)
        a, b, hout = self.a0.copy(), self.b0.copy(), np.full(max(nbytes, 1), HOST_FILL, np.uint8)
        if ops & H2D:
            a[64 + dst:64 + dst + nbytes] = self.hsrc[:nbytes]
        if ops & D2D:
            b[64 + dst:64 + dst + nbytes] = a[64 + src:64 + src + nbytes]
        if ops & FILL:
            b[64 + fo:64 + fo + nbytes] = value & 0xFF
        if ops & D2H:
            hout[:nbytes] = b[64 + src:64 + src + nbytes]
        self.want = (a, b, hout)

    def buffers(self):
        return np.full(len(self.a0), 0xEE, np.uint8), np.full(len(self.b0), 0xEE, np.uint8), np.full(max(self.nbytes, 1), HOST_FILL, np.uint8)

    def check(self, got, tag):
        for nm, g, w in zip(("A", "B", "host"), got, self.want):
            if not np.array_equal(g, w):
                bad = np.flatnonzero(g != w)
                raise AssertionError("%s: buffer %s differs in %d bytes, the first at %d (margins: [0, 64) and [%d, %d))"
                                     % (tag, nm, bad.size, bad[0], 64 + self.span, 128 + self.span))

    def tag(self):
        return "ops %d bytes %d dst %d src %d fill %d value %d" % (self.ops, self.nbytes, self.dst, self.src, self.fo, self.value)


def p8(a):
    return a.ctypes.data_as(U8)


def run_plain(lib, h, c):
    a, b, hout = c.buffers()
    rc = lib.asm_test_copy_fill(h, c.ops, c.span, c.nbytes, c.dst, c.src, c.fo, c.value, p8(c.a0), p8(c.b0), p8(c.hsrc), p8(hout), p8(a), p8(b))
    assert rc == 0, lib.asm_last_error(h)
    c.check((a, b, hout), "plain, " + c.tag())


def run_merged(lib, b, cases, expect_merged=True):
    Rec = _lib.hook_record("asm_test_copy_fill")
    keep, recs = [], (Rec * len(cases))()
    for r, c in zip(recs, cases):
        bufs = c.buffers()
        keep.append(bufs)
        for i, v in enumerate((c.ops, c.span, c.nbytes, c.dst, c.src, c.fo, c.value, p8(c.a0), p8(c.b0), p8(c.hsrc), p8(bufs[2]), p8(bufs[0]), p8(bufs[1]))):
            setattr(r, "a%d" % i, v)
    status = np.full(len(cases), -99, np.int32)
    merged.kernel_table(lib, b)
    rc = lib.asm_batch_test_run(b, _lib.TEST_FAMILIES.index("asm_test_copy_fill"), len(cases), C.cast(recs, C.c_void_p), _lib.i32ptr(status))
    merged.stop_after_device_error(lib, b, rc, status, "copy_fill")
    assert rc == 0, lib.asm_batch_last_error(b)
    assert not status.any(), status
    tab = merged.kernel_table(lib, b)
    for c, bufs in zip(cases, keep):
        c.check(bufs, "batch, " + c.tag())
    if expect_merged:
        # same byte counts, so the three scenarios' operations merge whatever their offsets: every launch serves all of them
        assert tab, "the batch recorded no kernel"
        for name, ops, launches, nb, gz in tab:
            assert ("k_bcopy" in name or "k_bfill" in name) and ops == len(cases) * launches and nb == len(cases) and gz == 1, (name, ops, launches, nb, gz)
        merged.note_merged(tab)
    return tab


PAIRS = list(itertools.product(OFFSETS, OFFSETS))
TRIPLES = [PAIRS[i::12] for i in range(12)]      # 12 triples of (dst, src): the three scenarios of a batch call mix aligned and unaligned offsets


@pytest.mark.parametrize("nbytes", COUNTS)
def test_copies_at_every_offset(hip_lib, handle, batch, nbytes):
    """H2D into A at dst, D2D from A + src to B + dst, D2H from B + src: every pair of offsets on the plain handle, in triples in the batch."""
    assert len(set(sum(TRIPLES, []))) == 36
    for dst, src in PAIRS:
        run_plain(hip_lib, handle, Case(H2D | D2D | D2H, nbytes, dst, src, seed=dst * 16 + src))
    for t in TRIPLES:
        tab = run_merged(hip_lib, batch, [Case(H2D | D2D | D2H, nbytes, dst, src, seed=100 + dst * 16 + src, span=nbytes + 12) for dst, src in t])
        assert any("k_bcopy" in r[0] for r in tab)


@pytest.mark.parametrize("value", VALUES)
def test_fills_at_every_offset(hip_lib, handle, batch, value):
    for nbytes in COUNTS:
        for fo in OFFSETS:
            run_plain(hip_lib, handle, Case(FILL, nbytes, fo=fo, value=value, seed=fo))
        for t in ((0, 1, 4), (2, 8, 12)):
            tab = run_merged(hip_lib, batch, [Case(FILL, nbytes, fo=fo, value=value, seed=50 + fo, span=nbytes + 12) for fo in t])
            assert any("k_bfill" in r[0] for r in tab)


@pytest.mark.parametrize("nbytes", [LOOP_64, LOOP_256, LOOP_64 + 4, LOOP_256 + 4], ids=["64wg-16B", "256wg-16B", "64wg-4B", "256wg-4B"])
def test_threads_loop_under_both_grid_caps(hip_lib, handle, batch, nbytes):
    """More 16-byte steps than 64 x 256 and than 256 x 256 threads.  A grid has min(cap, ceil(bytes / 16384)) workgroups, so the threads of
    every one of these counts make several passes of their grid-stride loop (1024 steps of 16 bytes per 256 threads); the larger count
    (65 workgroups asked for) is also cut to the recorded path's cap of 64.  The counts + 4 loop in the 4-byte branch.  All at offset 0; a
    fill of the same length follows the copies.  (The plain path's cap of 256: test_plain_grid_at_its_cap.)"""
    assert nbytes > (64 if nbytes < LOOP_256 else 256) * 256 * 16 and (nbytes % 16 == 0 or nbytes % 16 == 4)
    for ops, value in ((H2D | D2D | D2H, 0), (ALL, 0x1AB)):
        run_plain(hip_lib, handle, Case(ops, nbytes, value=value, seed=7))
        run_merged(hip_lib, batch, [Case(ops, nbytes, value=value, seed=8 + s) for s in range(3)])


@pytest.mark.parametrize("extra", [16, 20], ids=["16B", "4B"])
def test_plain_grid_at_its_cap(hip_lib, handle, extra):
    """256 x 16384 bytes and one step more ask for 257 workgroups: the plain path launches its cap of 256 and the last step is a second pass."""
    nbytes = 256 * 16384 + extra
    assert -(-nbytes // 16384) > 256
    run_plain(hip_lib, handle, Case(ALL, nbytes, value=0xAB, seed=11))


def test_looping_threads_in_different_branches_of_one_launch(hip_lib, batch):
    """Three scenarios of one byte count above the recorded grid's sweep at offsets 0, 4 and 1: the 4-byte count leaves the choice of the
    branch to the offsets."""
    run_merged(hip_lib, batch, [Case(H2D | D2D | D2H, LOOP_64 + 4, dst, src, seed=20 + dst, span=LOOP_64 + 16) for dst, src in ((0, 0), (4, 8), (1, 0))])
    run_merged(hip_lib, batch, [Case(FILL, LOOP_64 + 4, fo=fo, value=0xAB, seed=30 + fo, span=LOOP_64 + 16) for fo in (0, 4, 1)])


def test_zero_bytes_change_nothing(hip_lib, handle, batch):
    c = Case(ALL, 0, 4, 8, 12, 0xAB, seed=3, span=32)
    assert np.array_equal(c.want[0], c.a0) and np.array_equal(c.want[1], c.b0)
    run_plain(hip_lib, handle, c)
    tab = run_merged(hip_lib, batch, [c, Case(ALL, 0, seed=4, span=32), Case(ALL, 0, 1, 1, 1, -1, seed=5, span=32)], expect_merged=False)
    # only the loads and the read-backs of the buffers were recorded
    assert all("k_bcopy" in r[0] for r in tab)


def test_ranges_outside_the_buffer_are_refused(hip_lib, handle):
    a, b, hout = np.zeros(128 + 16, np.uint8), np.zeros(128 + 16, np.uint8), np.zeros(16, np.uint8)
    for ops, nbytes, dst, src, fo in ((D2D, 16, 1, 0, 0), (D2D, 16, 0, 1, 0), (FILL, 8, 0, 0, 9), (H2D, 17, 0, 0, 0), (D2H, 4, 0, -1, 0), (16, 4, 0, 0, 0), (FILL, -1, 0, 0, 0)):
        rc = hip_lib.asm_test_copy_fill(handle, ops, 16, nbytes, dst, src, fo, 0, p8(a), p8(b), p8(hout), p8(hout), p8(a), p8(b))
        assert rc == -1, (ops, nbytes, dst, src, fo, rc)
