"""The niceonly kernels' nice list, with something in it.

No nice number is known on any niceonly fast base, so every in-range list
comparison of the suite compared [] with []: the cube half of the digit test
(cube_pass: the ring read, cube_limbs and the LDS pair table, or the VALU path
of b65/68/80), the number emit_nice writes with its high word -- rebuilt from 12
packed bits plus a carry on the wide lane walk --, the ring's wrap and flush,
and the list's growth and re-run could all be wrong unseen.  Here
nice_debug_set_nice_min lowers the threshold the cube pass compares its count
with, so the production kernels list every square survivor whose digit union
has >= nice_min members, and every list is compared with the oracle's at the
same threshold (the restatement's for filter="sound").  The thresholds run
over every distinct union count of a window's survivors, so the nested lists
pin each survivor's exact count.  nice_min_windows.py holds the windows;
test_nice_min_hook.py checks on the CPU that none of them is empty.

Run on the MI355X box:  python -m pytest tests/test_gpu_nice_list.py -m gpu -q
"""
import ctypes
import random

import pytest

import nice_amd as N
from nice_amd import _lib
from oracle import oracle as O

import nice_min_windows as W
import sound_restatement as SR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = N.GpuContext(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _restore():
    """The oracle's Filter C switch and the hook are process-global."""
    yield
    O.lib().oracle_set_filter_c(1)
    for b in W.FAST:
        _lib.lib().nice_debug_set_nice_min(b, 0)


PATHS = {
    "host": ("fused", "host"),      # niceonly_kernel on host-built leaves
    "fused": ("fused", "device"),   # msd_fused_kernel + niceonly_kernel on the device's leaf list
    "wave": ("wave", "device"),     # msd_wave_kernel: narrow walk, wide walk (b57-62), packed groups (b65/68/80)
}


def totals(st, where):
    # (the host MSD path has no device counters: square_ok reads 0 there)
    return st.candidates, st.ranges, st.square_ok if where == "device" else 0


# --- a, e. every fast base x three paths, and production before and after ---------------------
@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("base", W.BASES)
def test_list_at_every_threshold(ctx, base, path):
    kind, where = PATHS[path]
    a, size, chunk = W.window(base, kind)
    ranges, cands, sq, surv = W.reference_field(a, size, base, chunk)
    assert len(surv) >= W.MIN_SURVIVORS and len({u for _, u in surv}) >= W.MIN_COUNTS
    if base >= 57:
        assert all(n >> 64 for n, _ in surv), "b >= 57: the comparison must cover the high word"
    opts = dict(chunk_size=chunk, msd_where=where)
    want_st = (cands, ranges, sq if where == "device" else 0)
    lst, st = ctx.niceonly_raw(a, a + size, base, **opts)
    assert lst == [] and totals(st, where) == want_st, "production, before the hook"
    ts = W.thresholds(surv)
    for t in ts:
        with W.lowered(base, t):
            lst, st = ctx.niceonly_raw(a, a + size, base, **opts)
        assert lst == W.listed(surv, t), (base, path, t, len(lst), len(W.listed(surv, t)))
        assert totals(st, where) == want_st and st.reruns == 0, (base, path, t)
        if t == ts[0]:
            # every square survivor exactly once: the ring's wrap and flush lose and repeat none
            assert len(lst) == sq == len(set(lst))
            if where == "device":
                assert len(lst) == st.square_ok
    assert W.listed(surv, ts[-1]) == []
    lst, st = ctx.niceonly_raw(a, a + size, base, **opts)
    assert lst == [] and totals(st, where) == want_st, "production, after the hook was cleared"
    print(f"b{base} {path}: {sq} survivors, thresholds {ts[0]}..{ts[-1]}")


# --- b. the sound variants --------------------------------------------------------------------------
@pytest.mark.parametrize("base,kind", [(b, "fused") for b in W.BASES] + [(b, "wave") for b in W.WAVE_WALKS])
def test_sound_list_at_every_threshold(ctx, base, kind):
    """SOUND instantiations: the list is the restatement's -- the candidates
    the prefix test keeps --, prefix_rejected does not move."""
    a, size, chunk = W.window(base, kind)
    surv = W.sound_survivors(a, size, base, chunk)
    ranges, cands, rej, sq, prod = SR.sound_field(a, size, base, chunk)
    assert len(surv) >= W.MIN_SURVIVORS and len({u for _, u in surv}) >= W.MIN_COUNTS and sq == len(surv)
    assert prod == [] and 0 < rej < cands
    if base >= 57:
        assert all(n >> 64 for n, _ in surv)
    opts = dict(chunk_size=chunk, msd_where="device", filter="sound")
    want_st = (ranges, cands, rej, sq)
    ts = W.thresholds(surv)
    for t in [0] + ts + [0]:
        with W.lowered(base, t):
            lst, st = ctx.niceonly_raw(a, a + size, base, **opts)
        assert lst == (W.listed(surv, t) if t else []), (base, kind, t)
        assert (st.ranges, st.candidates, st.prefix_rejected, st.square_ok) == want_st, (base, kind, t)
        if t == ts[0]:
            assert len(lst) == st.square_ok == len(set(lst))


# --- c. the cube pass's count, per n -----------------------------------------------------------------
def cube_cases(base):
    """n and the count the cube pass must see: the union count where n^2 is
    repeat-free, else 0."""
    s, e = O.base_range(base)
    d2 = len(SR.digits(s * s, base))
    rng = random.Random(6400 + base)
    drawn, free = [], []
    while len(free) < 30:
        assert len(drawn) < 400_000, "the rate of repeat-free squares fell below 1 in 1e4"
        batch = [rng.randrange(s, e) for _ in range(20_000)]
        drawn += batch
        # the oracle's scan passes the square's d2 digits: no repeat among them
        free += [n for n in batch if O.scan_depth(n, base) > d2]
    edges = [s, s + 1, e - 2, e - 1]
    # both sides of every 32-bit word boundary of n, n^2 and n^3 inside the range
    for p in (1, 2, 3):
        for w in range(32, 128 * p + 1, 32):
            x = root_ceil(1 << w, p)  # the first n with n^p >= 2^w
            edges += [n for n in range(x - 2, x + 3) if s <= n < e]
    ns = free + drawn[:300] + edges
    want = [O.num_unique_digits(n, base) if SR.square_repeat_free(n, base) else 0 for n in ns]
    assert all(SR.square_repeat_free(n, base) for n in free) and sum(1 for u in want if u) >= 30
    assert sum(1 for u in want if not u) >= 200
    return ns, want


def root_ceil(v, p):
    """The least x with x^p >= v."""
    lo, hi = 0, 1 << (v.bit_length() // p + 1)
    while lo < hi:
        mid = (lo + hi) // 2
        if mid ** p >= v:
            hi = mid
        else:
            lo = mid + 1
    return lo


@pytest.mark.parametrize("base", W.FAST)
def test_cube_count_per_n(ctx, base):
    """nice_debug_cube_count, b64 included (which no field reaches): seeded
    random in-range n with repeat-free squares, a few hundred unfiltered ones,
    the range ends and the word boundaries of n, n^2, n^3."""
    ns, want = cube_cases(base)
    got = ctx.debug_cube_count(ns, base)
    bad = [(n, g, w) for n, g, w in zip(ns, got, want) if g != w]
    assert not bad, (base, len(bad), bad[:5])
    s, e = O.base_range(base)
    for n in (s - 1, e):
        with pytest.raises(N.NiceError):
            ctx.debug_cube_count([s, n], base)
    with pytest.raises(N.NiceError):
        ctx.debug_cube_count([O.base_range(70)[0]], 70)


# --- d. growth and re-run ------------------------------------------------------------------------------
def grow_want(chunk):
    a, size = W.GROW_FIELD
    surv = W.reference_field(a, size, 40, chunk)[3]
    assert len(surv) > 2 ** 16
    return a, a + size, [n for n, _ in surv], W.reference_field(a, size, 40, chunk)[:3]


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("chunk", [10 ** 6, 10 ** 8])
def test_list_growth_reruns_the_field(chunk, where):
    """A fresh context's device list holds 2^16 entries; the b40 2e9 field at
    nice_min 1 lists 170 413 (1e8 chunks: the wave kernel) or about as many
    (1e6 chunks: fused): the field runs again on the grown list, once, and a
    later field on a grown list does not."""
    a, e, want, (ranges, cands, sq) = grow_want(chunk)
    c = N.GpuContext(0)
    try:
        with W.lowered(40, 1):
            # a context rotates its fields over three slots, each with a list of its own:
            # three fields grow one each, the fourth finds the first slot's list grown
            # (cap: room for the whole list, so that no call is repeated for want of room)
            for reruns in (1, 1, 1, 0):
                lst, st = c.niceonly_raw(a, e, 40, chunk_size=chunk, msd_where=where, cap=len(want) + 1)
                assert lst == want and st.reruns == reruns
                assert totals(st, where) == (cands, ranges, sq if where == "device" else 0)
    finally:
        c.close()


@pytest.mark.parametrize("where", ["device", "host"])
def test_list_growth_on_two_devices(where):
    a, e, want, (ranges, cands, sq) = grow_want(10 ** 8)
    two = N.GpuContext([0, 0])
    try:
        with W.lowered(40, 1):
            lst, st = two.niceonly_raw(a, e, 40, chunk_size=10 ** 8, msd_where=where, cap=len(want) + 1)
        assert lst == want and st.reruns >= 1
        assert totals(st, where) == (cands, ranges, sq if where == "device" else 0)
    finally:
        two.close()


def test_submit_collect_capacity_and_captured_threshold():
    """Through submit / collect with a caller list of 16 entries:
    NICE_ERR_CAPACITY with the true length, then the list.  The threshold is
    the one at submit: the hook is cleared before the collect, whose re-run
    must keep it; a field submitted after the clearing is production's."""
    a, e, want, _ = grow_want(10 ** 8)
    L = _lib.lib()
    c = N.GpuContext(0)
    try:
        opts = N.GpuContext._nice_opts(chunk_size=10 ** 8, msd_where="device")
        t = ctypes.c_int()
        with W.lowered(40, 1):
            _lib.check(L.nice_niceonly_submit(c._h, *O._split(a), *O._split(e), 40, opts, t))
        t2 = c.niceonly_submit(a, e, 40, chunk_size=10 ** 8, msd_where="device")
        small, n, st = (_lib.nice_number * 16)(), ctypes.c_size_t(), _lib.nice_niceonly_stats()
        assert L.nice_niceonly_collect(c._h, t.value, small, 16, n, st) == _lib.NICE_ERR_CAPACITY
        assert n.value == len(want) and st.reruns == 1
        big = (_lib.nice_number * n.value)()
        _lib.check(L.nice_niceonly_collect(c._h, t.value, big, n.value, n, st))
        assert [big[i].number_lo | (big[i].number_hi << 64) for i in range(n.value)] == want
        assert st.reruns == 1 and all(big[i].num_uniques == 40 for i in range(0, n.value, 997))
        lst, st2 = c.niceonly_collect(t2)
        assert lst == [] and st2.reruns == 0 and st2.square_ok == st.square_ok
    finally:
        c.close()


# --- e. what the hook must not touch --------------------------------------------------------------------
def test_out_of_range_and_other_bases_keep_production(ctx):
    """With the hook at b40's lowest threshold: a b40 field across the start
    of the range (not wholly in range: the generic digit test) and b10's
    [47, 100) return their production lists."""
    r0, _ = O.base_range(40)
    # (the first square survivors of b40's range lie 8.3e8 above its start)
    chunk = 10 ** 7
    a, e = r0 - chunk, r0 + 85 * chunk
    res, cands, ranges, _ = O.process_field_niceonly_sq(a, e, 40, W.THREADS, chunk)
    inside = O.process_field_niceonly_sq(r0, e, 40, W.THREADS, chunk, nice_min=1)[0].nice_numbers
    assert len(inside) >= W.MIN_SURVIVORS, "the in-range part must have something to list"
    with W.lowered(40, 1):
        for where in ("device", "host"):
            lst, st = ctx.niceonly_raw(a, e, 40, chunk_size=chunk, msd_where=where)
            assert lst == [n for n, _ in res.nice_numbers] == []
            assert (st.candidates, st.ranges) == (cands, ranges)
        assert ctx.niceonly_raw(47, 100, 10)[0] == [69]
        assert ctx.niceonly_raw(r0, e, 40, chunk_size=chunk, msd_where="device")[0] == [n for n, _ in inside]


@pytest.mark.parametrize("base,kind", [(40, "fused"), (57, "wave"), (80, "wave")])
def test_dealt_runs_concatenate(ctx, base, kind):
    a, size, chunk = W.window(base, kind)
    surv = W.reference_field(a, size, base, chunk)[3]
    with W.lowered(base, 1):
        parts = [ctx.niceonly_raw(a, a + size, base, chunk_size=chunk, msd_where="device", deal_stride=2,
                                  deal_offset=r)[0] for r in range(2)]
    want = [[n for n, _ in surv if (n - a) // chunk % 2 == r] for r in range(2)]
    assert all(want) and parts == want
