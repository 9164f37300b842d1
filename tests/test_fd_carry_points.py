"""The deep-carry points of tests/fd_carry_points.py, the parts that need no
GPU: every point is a crossing, lies inside its limb layout, every layout has
points of all four quantities down to the deepest level its numbers reach, and
the windows the GPU tests run put each point in the middle of one lane's run
(by the map plan and the batch plan, without a device).
"""
import pytest

from oracle import oracle as O

import fd_carry_points as F
import near_miss_windows as W
from test_map import FD, plan as map_plan
from test_ranges import plan as ranges_plan

BASES = W.fd_bases()


def digits(x, radix):
    out = []
    while x:
        x, d = divmod(x, radix)
        out.append(d)
    return out  # least significant first


def deepest_changed_limb(x, y, base):
    """The highest radix-b^2 limb in which x < y differ: the deepest level a
    quantity growing from x to y crosses."""
    dx, dy = digits(x, base * base), digits(y, base * base)
    dx += [0] * (len(dy) - len(dx))
    return max(i for i in range(len(dy)) if dx[i] != dy[i])


def test_the_bases_are_the_fd_bases():
    assert len(BASES) == 24 and BASES[0] == 40 and BASES[-1] == 80
    assert sorted(W.WINDOW_FRAC) == BASES
    assert sum(len(F.intervals(b)) for b in BASES) == 37  # the instantiations of fd2_combos.h


@pytest.mark.parametrize("base", BASES)
def test_points_are_deep_crossings_inside_their_layout(base):
    B = base * base
    rs, re = O.base_range(base)
    ivs = F.intervals(base)
    assert F.layout_cuts(base) == W.cuts_of(base)
    assert ivs[0][0] == rs and ivs[-1][1] == re and all(x[1] == y[0] for x, y in zip(ivs, ivs[1:]))
    pts = F.points(base)
    assert 10 <= len(pts) <= 74
    seen = set()
    for iv, q, k, n in pts:
        a, e = iv
        assert iv in ivs and (iv, q, k) not in seen and k >= 1
        seen.add((iv, q, k))
        Q = F.QUANTITIES[q]
        # the crossing identity, spelt out
        assert Q(n) // B ** k == Q(n - 1) // B ** k + 1, (base, q, k, n)
        assert a + F.MARGIN <= n <= e - F.MARGIN - 1, (base, q, k, n)
        # rarer than once per 1e6 numbers of the interval
        assert (Q(e - 1) // B ** k - Q(a) // B ** k) * F.RARE < e - a
    for iv in ivs:
        a, e = iv
        for q, Q in F.QUANTITIES.items():
            levels = sorted(k for i, qq, k, _ in pts if i == iv and qq == q)
            assert levels, (base, iv, q)
            assert levels == list(range(levels[0], levels[-1] + 1)), (base, iv, q, levels)
            # the deepest level the interval's numbers (a margin inside) reach, from their limbs
            assert levels[-1] == deepest_changed_limb(Q(a + F.MARGIN - 1), Q(e - F.MARGIN - 1), base), (base, iv, q)
            # the level below the shallowest kept one is frequent: nothing rare was left out
            k = levels[0] - 1
            assert k == 0 or (Q(e - 1) // B ** k - Q(a) // B ** k) * F.RARE >= e - a, (base, iv, q)


@pytest.mark.parametrize("base", BASES)
def test_deepest_levels_from_the_digit_counts(base):
    """Inside the valid range n^2 has ds and n^3 dc base-b digits, ds + dc = b:
    n^2 fills NS = ceil(ds / 2) limbs and n^3 NC = ceil(dc / 2), and the deepest
    point steps their top limbs, NS - 1 and NC - 1.  2n+1 and 3n+1 reach their
    top limb too: the limb count at the range's end less one, or -- where the
    only crossing of that level is the limb-layout cut itself (2n+1 = B^k IS a
    cut, and no lane steps across a cut) -- one level lower."""
    rs, re = O.base_range(base)
    ds, dc = len(digits(rs * rs, base)), len(digits(rs ** 3, base))
    assert ds + dc == base and (ds, dc) == (len(digits((re - 1) ** 2, base)), len(digits((re - 1) ** 3, base)))
    top = {q: max(k for _, qq, k, _ in F.points(base) if qq == q) for q in F.QUANTITIES}
    assert top["S"] == (ds + 1) // 2 - 1
    assert top["C"] == (dc + 1) // 2 - 1
    B = base * base
    for q in ("D1", "N3"):
        Q = F.QUANTITIES[q]
        nl = F.limbs(Q(re - 1), base)
        second = 2 * B ** (nl - 1)  # the first multiple of B^(nl-1) whose crossing is not a change of limb count
        want = nl - 1 if Q(rs + F.MARGIN) < second <= Q(re - F.MARGIN - 1) or F.limbs(Q(rs), base) == nl else nl - 2
        assert top[q] == want, (base, q, nl)
    if base == 80:  # the table of the module text
        per = {(i, q): [k for iv, qq, k, _ in F.points(80) if iv == F.intervals(80)[i] and qq == q]
               for i in range(3) for q in F.QUANTITIES}
        assert all(per[i, "S"] == list(range(10, 16)) and per[i, "C"] == list(range(18, 24)) for i in range(3))
        assert all(per[i, "D1"][0] == 2 and per[i, "N3"][0] == 2 for i in range(3))
        assert len(F.points(80)) == 74


def wg_of(base):
    """The workgroup size of the base's map and batch kernels, from their plans."""
    rs, _ = O.base_range(base)
    wg = max(r[3] for r in map_plan(base, rs, rs + 10 ** 6))
    assert wg in (512, 1024) and wg == ranges_plan(base, [(rs, rs + 10 ** 6)])[0][1]
    return wg


@pytest.mark.parametrize("base", BASES)
def test_windows_put_each_point_inside_one_lanes_run(base):
    """The map window and the two batch windows of every point: one FD segment,
    and n* in a main workgroup, at least two numbers from either end of its
    lane's run -- so the lane steps n*-1 -> n* and at least two numbers more."""
    wg = wg_of(base)
    chunk = 41 if wg == 512 else 21
    rs, _ = O.base_range(base)
    assert map_plan(base, rs, rs + F.WINDOW)[0][4] == chunk
    ranges, stars = [], []
    for _, q, k, n in F.points(base):
        a = F.window_for(n, chunk)
        recs = map_plan(base, a, a + F.WINDOW)
        assert all(r[0] == FD for r in recs) and len({r[5] for r in recs}) == 1, (base, q, k)
        assert sum(1 for r in recs if r[4] == 1) == 1 and recs[-1][4] == 1  # one segment: one tail workgroup
        mine = [r for r in recs if r[1] <= n < r[1] + r[6]]
        assert len(mine) == 1 and mine[0][4] == chunk >= 21 and mine is not recs[-1], (base, q, k)
        off = (n - mine[0][1]) % chunk
        assert 2 <= off <= chunk - 3 and off == chunk // 2 and (n - mine[0][1]) // chunk == F.LANE
        ranges += [(a, a + F.WINDOW), (a - 1, a - 1 + F.WINDOW)]
        stars += [n, n]
    units = ranges_plan(base, ranges)
    for ri, n in enumerate(stars):
        mine = [u for u in units if u[3] == ri]
        assert len({u[4] for u in mine}) == 1 and sum(1 for u in mine if u[2] == 1) == 1
        hold = [u for u in mine if u[0] <= n < u[0] + u[1] * u[2]]
        assert len(hold) == 1 and hold[0][2] == chunk, (base, ri)
        off = (n - hold[0][0]) % chunk
        assert 2 <= off <= chunk - 3 and off == chunk // 2 + ri % 2


def test_window_for():
    assert F.window_for(10 ** 6, 41) == 10 ** 6 - 4120 and F.window_for(10 ** 6, 21, lane=3) == 10 ** 6 - 73
