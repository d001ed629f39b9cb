"""-m gpu: zn_gemm's peeled last chunk and its class-table epilogue (conp_zn.hip) at their edges.

The last chunk of a range carries the first batch of the class table P (CB = 3 classes in flight) in the gaps between its MFMAs, and
the epilogue requests class cb + CB + k as soon as class cb + k's products are formed.  Every case runs the z-window path through
the entry points of tests/test_gpu_zwindow.py (FixConp.b_cal, capi.test_paths) and compares b with the full contraction's
(CONP_PATH_SK_CLASSIC) of the same handle arguments at that file's bar, 1e-11 of the largest entry.  Each case first asserts on the
host side -- fx.info() and the list arithmetic of conp_fix.cpp's zn_build_items restated here -- that it takes the path and has the
property it is named for, and skips with a message otherwise.

What the host plan does not let one rank reach: the planner keeps at least six chunks per range, so ranges of one, two and four
chunks are a rank's share of the chunk axis among many ranks (the share of rank r of W is the r-th W-th of the chunks: conp_fix.cpp,
"shares are fractions"), checked against a range of eight chunks over the same atoms; a single z class needs both electrodes in
one plane."""
import numpy as np
import pytest

from conp_amd import FixConp, capi, neighbor, systems
from helpers import rel_err

pytestmark = pytest.mark.gpu
B_BAR = 1e-11                                              # tests/test_gpu_zwindow.py, the same comparison


def _medium(mode="ffield", seed=7, **kw):
    a = dict(n_cells_x=16, n_cells_y=8, lz=300.0, n_elyte=16384, cutoff=12.0, accuracy_relative=1e-6, g_ewald=0.26, mode=mode,
             seed=seed)
    a.update(kw)
    return systems.synthetic_fast(**a)


def _lift_half_a_sheet(s):
    """half of the lowest electrode sheet lifted by 1 A: one z class more"""
    sheet = np.nonzero(s.echeck == 1)[0]
    outer = sheet[s.x[sheet, 2] < s.x[sheet, 2].min() + 0.1]
    s.x[outer[: len(outer) // 2], 2] += 1.0
    return s


def _one_plane():
    """both electrodes in ONE plane (the second one moved onto the first one's z, half a lattice spacing aside): one z class"""
    s = _medium(seed=83)
    a, b = s.echeck == 1, s.echeck == -1
    za = np.unique(np.round(s.x[a, 2], 6))
    assert len(za) == 1
    d = np.sort(np.unique(np.round(s.x[a, 0], 6)))
    s.x[b, 2] = s.x[a, 2][0]
    s.x[b, 0] += 0.5 * (d[1] - d[0])
    return s


def _rough():
    s = _medium(seed=23)
    ele = s.echeck != 0
    s.x[ele, 2] += np.random.default_rng(23).uniform(-0.4, 0.4, size=int(ele.sum()))
    return s


def _shifted(s, dz):
    """the whole system translated along z and wrapped into the box"""
    lo = s.boxlo[2]
    s.x[:, 2] = lo + np.mod(s.x[:, 2] - lo + dz, s.prd[2])
    return s


def _sort_origin(s, n):
    """zn_order_list (conp_fix.cpp) restated: the listed atoms' grid cells (u = z n / Lz modulo n), the cell behind the longest run
    of empty cells (c_start, 0 in a box without an empty cell), the cells relative to it in ascending order"""
    z = s.x[(s.echeck == 0) & (s.q != 0), 2]
    u = z * (n / s.prd[2])
    cell = np.minimum((u - n * np.floor(u / n)).astype(int), n - 1)
    occ = np.bincount(cell, minlength=n)
    best_len = best_end = run = 0
    for c in range(2 * n):
        if occ[c % n] == 0:
            run += 1
            if run > best_len and run <= n:
                best_len, best_end = run, c % n
        else:
            run = 0
    c_start = (best_end + 1) % n if best_len > 0 else 0
    return c_start, np.sort(np.mod(cell - c_start, n))


def _origins(s, n, nr):
    """zn_build_items restated: the window origin g0 = c_start + imin - margin of every range, imin the lowest first tap
    ceil(u - 7.5) of its atoms -- cell - 7 or cell - 6 for the atoms of the range's lowest cell, so g0 is G or G + 1; returns G"""
    c_start, rel = _sort_origin(s, n)
    margin = int(np.ceil(2.5 / (s.prd[2] / n)))
    nchunks = (len(rel) + 15) // 16
    return c_start, margin, [c_start + int(rel[16 * (nchunks * r // nr)]) - 7 - margin for r in range(nr)]


def _b(s, at, alist, blist, mask, rank=0, nranks=1):
    with capi.test_paths(mask):
        fx = FixConp(s, rank=rank, nranks=nranks)
        fx.init_lists(alist, blist)
        fx.setup_post_neighbor(at)
        fx.b_cal(at)
        b = fx.vectors()[0].copy()
        info = fx.info()
        out = (b, info.zn_cols, info.n_zclasses, info.n_elyte_charged, info.zn_rows, info.zn_grid,
               (info.kcount_flat,) + tuple(info.kcount_dims)[:3])
        fx.close()
    return out


def _compare(s, label, cols, nzc, mask=0, rank=0, nranks=1):
    at, alist, blist = neighbor.build_lists(s)
    b_zn, c_zn, k_zn, nl, rows, grid, kc = _b(s, at, alist, blist, mask, rank, nranks)
    if c_zn not in cols or k_zn != nzc:
        pytest.skip(f"{label}: the handle planned zn_cols {c_zn} with {k_zn} z classes, the case needs {cols} and {nzc}")
    b_cl, c_cl = _b(s, at, alist, blist, mask | capi.PATH_SK_CLASSIC, rank, nranks)[:2]
    assert c_cl == 0
    assert np.abs(b_cl).max() > 0
    e = rel_err(b_zn, b_cl)
    print(f"{label}: zn_cols {c_zn} grid {grid} nzc {k_zn} charged {nl} rows {rows}: b {e:.2e} of max")
    assert e < B_BAR, (label, e)
    return dict(nl=nl, rows=rows, grid=grid, cols=c_zn, kcounts=kc)


def _n_ranges(nchunks, nrt, cols):
    """zn_build_items on one rank: ranges = slots per CU (four with 32 columns, three with 48) x CUs / row tiles x rounds, capped at
    one per six chunks.  Where the cap binds with one round -- these systems' 1024 chunks on a part of 256 CUs -- every candidate
    of the planner with as many slots gives the same count."""
    import torch
    cap = max(1, nchunks // 6)
    nr = min(max(1, (4 if cols == 32 else 3) * torch.cuda.get_device_properties(0).multi_processor_count // nrt), cap)
    if nr != cap:
        pytest.skip(f"{nrt} row tiles on this part: fewer than {cap} ranges, their count depends on the candidate the planner took")
    return nr


def _tile_kinds(kcounts):
    """KPlan::build (conp_host.cpp) restated: the row tiles [0, lo) hold the singles (the origin, the x and the y axis vectors)
    filled up with pairs, [lo, hi) hold 32 whole (+ky, -ky) pairs each (ZnItem::paired)"""
    flat, d0, d1, d2 = kcounts
    singles, pairs = 1 + d0 + d1, flat - d0 - d1 - d2
    singles -= singles % 2                                 # (an odd one out goes to the end)
    fill = min((64 - singles % 64) % 64, pairs)
    lo = (singles + fill) // 64
    hi = lo + ((pairs - fill) // 64 if (singles + fill) % 64 == 0 else 0)
    return lo, hi


# ---- the class batches: one partial batch, exactly CB, CB + 1, two full batches (and the decks' two) ----------------------------
@pytest.mark.parametrize("nzc", [1, 2, 3, 4, 6])
def test_class_batches(nzc):
    """nzc = 1: the clamp min(k, nzc - 1) of the prefetched batch and the store guard; 3: exactly one batch, no second request;
    4: a second batch of one class (the clamp of the rolling request); 6: two full batches.  On one rank the ranges of this size
    hold 6 or 7 chunks (1024 chunks over 170 ranges, one per six chunks): an odd and an even count, i.e. both panel buffers under
    the peeled chunk, in every one of these cases; the head row tile is a tile of singles, the others hold pairs."""
    if nzc == 1:
        s = _one_plane()
    elif nzc == 3:
        s = _lift_half_a_sheet(_medium(seed=89))
    else:
        s = _medium(layers=nzc // 2, seed=40 + nzc)
    h = _compare(s, f"nzc {nzc}", (32, 48), nzc)
    nchunks, nrt = (h["nl"] + 15) // 16, h["rows"] // 128
    nr = _n_ranges(nchunks, nrt, h["cols"])
    lens = {nchunks * (r + 1) // nr - nchunks * r // nr for r in range(nr)}
    lo, hi = _tile_kinds(h["kcounts"])
    print(f"nzc {nzc}: {nchunks} chunks, {nr} ranges of {sorted(lens)} chunks; {nrt} row tiles, pairs in [{lo}, {hi})")
    assert lo >= 1 and lo < hi <= nrt, "a head tile of singles and at least one tile of whole pairs"
    assert any(n & 1 for n in lens) and any(not n & 1 for n in lens), "an odd and an even chunk count"


# ---- the shortest ranges: the peeled chunk is also the first; both panel parities ----------------------------------------------
def test_short_ranges_add_up_to_a_long_one():
    """Ranks whose share of the chunk axis is one, two and four chunks run one range each (fewer than six chunks): the loop runs
    zero, one and three bodies before the peeled chunk, which reads panel 0, panel 1, panel 1; with one chunk it is also the first.
    The full form cuts a rank's share differently (per tile), so a single rank's b has no full-form counterpart; the reference is
    the same stretch of eight chunks as ONE range of a rank with eight chunks (a loop of seven bodies, the lengths the planner
    makes on one rank, which test_class_batches pins to the full form): the shares' b vectors add up to it, as the all-reduce of
    b adds them (tests/test_gpu_zwindow.py::test_z_window_rank_shards_add_up, its bar)."""
    s = _medium(seed=7)
    at, alist, blist = neighbor.build_lists(s)
    nl = int(np.count_nonzero((s.echeck == 0) & (s.q != 0)))
    nchunks = (nl + 15) // 16
    if nchunks % 8:
        pytest.skip(f"{nchunks} chunks do not split into shares of eight")
    w8 = nchunks // 8
    r8 = w8 // 3
    b8, c8, _, nl_h = _b(s, at, alist, blist, 0, r8, w8)[:4]
    assert nl_h == nl and c8 in (32, 48) and np.abs(b8).max() > 0
    for per_rank in (1, 2, 4):
        world, total = nchunks // per_rank, np.zeros_like(b8)
        for r in range(r8 * 8 // per_rank, (r8 + 1) * 8 // per_rank):
            assert nchunks * (r + 1) // world - nchunks * r // world == per_rank          # the share of rank r, in chunks
            b, c = _b(s, at, alist, blist, 0, r, world)[:2]
            assert c in (32, 48), f"rank {r} of {world} did not take the z-window path"
            total += b
        e = rel_err(total, b8)
        print(f"{8 // per_rank} ranges of {per_rank} chunk(s) against one of eight: b {e:.2e} of max")
        assert e < 1e-12, (per_rank, e)


# ---- 48 columns, the periodic wrap, the raw windows --------------------------------------------------------------------------------
def test_48_columns_four_classes():
    """NCF = 3: twelve columns per lane and class, 36 loads in the peeled chunk's gaps; two batches"""
    _compare(_medium(layers=2, seed=47), "48 columns", (48,), 4, mask=capi.PATH_ZN_WIDE)


@pytest.mark.parametrize("case", ["origin below 0", "origin at or above n"])
def test_windows_across_the_periodic_boundary(case):
    """The scalar residue of a window origin outside [0, n) and the lanes' one conditional subtraction, against the full contraction.
    "origin below 0": the system is moved so that the liquid begins two cells above grid point 0 (c_start = 2): the head range's
    origin 2 - 7 - margin is negative (the `gb < 0` branch behind the scalar remainder) and its window runs across n from below.
    "origin at or above n": the box of tests/test_gpu_zwindow.py's wrap test, the liquid across the box's upper face: c_start is in
    mid-box and the tail ranges' origins c_start + imin - margin pass n.  Both are asserted from the host's list arithmetic."""
    from test_zwindow_math import zn_grid_of
    s = _medium(seed=19)
    n = zn_grid_of(s)
    assert s.slabflag == 0                                 # (the grid spans the box itself: u = z n / Lz)
    if case == "origin below 0":
        c0, _ = _sort_origin(s, n)
        s = _shifted(s, -(c0 - 2) * s.prd[2] / n)
    else:
        s = _shifted(s, 0.37 * s.prd[2])
    h = _compare(s, case, (32, 48), 2)
    assert h["grid"] == n
    ncol = h["cols"]
    c_start, margin, G = _origins(s, n, _n_ranges((h["nl"] + 15) // 16, h["rows"] // 128, ncol))
    below = [g for g in G if g + 1 < 0]
    above = [g for g in G if g >= n]
    across = [g for g in G if n - ncol + 1 <= g % n <= n - 2]      # g0 = G or G + 1: columns below n AND columns at or above it
    print(f"{case}: n {n} c_start {c_start} margin {margin}: origins {min(G)} .. {max(G)} (+ 0 or 1); {len(below)} below 0, "
          f"{len(above)} at or above n, {len(across)} windows across n")
    if case == "origin below 0":
        assert c_start - 6 - margin < 0 and below, "no window origin below 0"
    else:
        assert above, "no window origin at or above n"
    assert across, "no window across n"


def test_raw_windows_once():
    """zn_gemm<RAW>: the peeled chunk without the table fetch, the store epilogue as it was"""
    _compare(_rough(), "rough", (32, 48), 0)
