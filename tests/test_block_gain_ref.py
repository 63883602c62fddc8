"""CPU: block gain compensation without a GPU -- the numpy restatement (tests/block_gain_ref.py) against tests/gain_ref.py on the 10-frame
case of tests/test_gpu_gain.py, mi355_solve_block_gains (host only) against the dense numpy solution, the smoothing, every refusal of the solve,
and the vignetting inputs' ranking (block-compensated < frame-compensated < uncompensated) on the restatement alone."""
import numpy as np
import pytest

from tests import block_gain_ref as br
from tests import gain_ref as gr


@pytest.fixture(scope="module")
def ten(oracle):
    imgs, h9s, pairs = br.ten_frames()
    sizes = [(i.shape[1], i.shape[0]) for i in imgs]
    coords, _ = br.coord_maps(sizes, h9s)
    return imgs, h9s, pairs, sizes, coords, gr.frame_sample_maps(oracle, imgs, h9s)


def test_coordinates_give_the_oracles_cover_and_samples(ten):
    imgs, h9s, pairs, sizes, coords, maps = ten
    own = br.sample_maps(imgs, coords)
    for k in range(len(imgs)):
        assert (coords[k] is None) == (maps[k] is None)
        if maps[k] is not None:
            assert np.array_equal(coords[k][2], maps[k][1]), k
            assert np.array_equal(own[k][0][own[k][1]], maps[k][0][maps[k][1]]), k


@pytest.mark.parametrize("step,gx,gy", [(1, 4, 3), (4, 5, 7), (8, 16, 16)])
def test_sums_over_cells_equal_gain_ref(ten, step, gx, gy):
    imgs, h9s, pairs, sizes, coords, maps = ten
    recs, cover = br.stats_ref(maps, coords, sizes, pairs, step, gx, gy)
    ref, cov_ref = gr.stats_ref(maps, pairs, step)
    assert np.array_equal(cover.sum(axis=1), cov_ref)
    assert np.all(recs["n"] > 0)
    for p in range(len(pairs)):
        m = recs["pair"] == p
        assert int(recs["n"][m].sum()) == ref[p][0]
        assert np.array_equal(recs["sum_a"][m].sum(axis=0), ref[p][1]) and np.array_equal(recs["sum_b"][m].sum(axis=0), ref[p][2])
    assert len(recs) > len(pairs)                                  # more than one cell combination per pair


@pytest.mark.parametrize("channels", [1, 3])
def test_grid_one_gives_gain_refs_normal_equations(ten, channels):
    imgs, h9s, pairs, sizes, coords, maps = ten
    recs, cover = br.stats_ref(maps, coords, sizes, pairs, 4, 1, 1)
    ref, cov_ref = gr.stats_ref(maps, pairs, 4)
    mine = br.normal_equations(recs, pairs, cover, channels=channels)
    theirs = gr.normal_equations(gr.to_records(ref, pairs), cov_ref, channels=channels)
    for (A, b), (A2, b2) in zip(mine, theirs):
        assert np.array_equal(A, A2) and np.array_equal(b, b2)


def random_records(n, gx, gy, seed, density=0.5, dead=()):
    """a chain of n frames plus some chords; per pair a random subset of the cell combinations; `dead`: nodes (frame, cell) with no cover and no record"""
    rng = np.random.default_rng(seed)
    cells = gx * gy
    pairs = [(k, k + 1) for k in range(n - 1)] + [(k, k + 3) for k in range(0, n - 3, 2)]
    node_gain = rng.uniform(0.8, 1.2, (n, cells))
    dead = set(dead)
    recs = []
    for p, (a, b) in enumerate(pairs):
        for ca in range(cells):
            for cb in rng.choice(cells, max(1, int(density * min(cells, 6))), replace=False):
                if (a, ca) in dead or (b, int(cb)) in dead:
                    continue
                r = np.zeros((), br.REC)
                nn = int(rng.integers(1, 400))
                base = rng.uniform(60, 180, 3)
                r["pair"], r["cell_a"], r["cell_b"], r["n"] = p, ca, cb, nn
                r["sum_a"] = np.round(base * node_gain[a, ca] * nn); r["sum_b"] = np.round(base * node_gain[b, cb] * nn)
                recs.append(r)
    recs = np.sort(np.array(recs, br.REC), order=["pair", "cell_a", "cell_b"])
    cover = rng.integers(50, 900, (n, cells)).astype(np.int64)
    for k, c in dead:
        cover[k, c] = 0
    return recs, pairs, cover


def rel_err(g, ref):
    return float(np.max(np.abs(np.asarray(g, np.float64) - ref)) / np.max(np.abs(ref)))


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("n,gx,gy", [(12, 1, 1), (8, 4, 3), (4, 16, 16)])
def test_solve_matches_numpy(lib, n, gx, gy, channels):
    recs, pairs, cover = random_records(n, gx, gy, seed=gx + channels)
    g = lib.solve_block_gains(recs, pairs, cover, grid_x=gx, grid_y=gy, smooth=0, channels=channels)
    ref = br.solve_ref(recs, pairs, cover, gx, gy, channels=channels)
    assert g.dtype == np.float32 and g.shape == (n, gy, gx, 3)
    # 1e-9 of the exact solution is the contract; a float32 output can show it to within one float ulp of the exact value
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(g.astype(np.float64) - ref) <= ulp)
    assert lib.solve_block_gains(recs, pairs, cover, grid_x=gx, grid_y=gy, smooth=0, channels=channels).tobytes() == g.tobytes()
    if channels == 1:
        assert np.array_equal(g[..., 0], g[..., 1]) and np.array_equal(g[..., 0], g[..., 2])


def test_grid_one_equals_the_per_frame_solve(lib):
    recs, pairs, cover = random_records(12, 1, 1, seed=3)
    st = np.zeros(len(recs), lib.GAIN_PAIR_STATS)
    ab = np.asarray(pairs)
    st["a"], st["b"] = ab[recs["pair"], 0], ab[recs["pair"], 1]
    st["n"], st["sum_a"], st["sum_b"] = recs["n"], recs["sum_a"], recs["sum_b"]
    g = lib.solve_block_gains(recs, pairs, cover, grid_x=1, grid_y=1, smooth=0)
    assert np.array_equal(g.reshape(12, 3), lib.solve_gains(st, cover.reshape(-1)))


def test_large_system_iterates_to_the_same_solution(lib):
    """a graph whose envelope the factorisation would not take (every frame paired with every other at 16 x 16 cells: 3072 unknowns, an
    almost full envelope) goes through the conjugate gradient, and meets the same bound"""
    n, gx, gy = 12, 16, 16
    cells = gx * gy
    rng = np.random.default_rng(8)
    pairs = [(a, b) for a in range(n) for b in range(a + 1, n)]
    recs = np.zeros(len(pairs) * cells, br.REC)
    recs["pair"] = np.repeat(np.arange(len(pairs)), cells)
    recs["cell_a"] = np.tile(np.arange(cells), len(pairs))
    recs["cell_b"] = rng.integers(0, cells, len(recs))
    recs["n"] = rng.integers(1, 300, len(recs))
    base = rng.uniform(60, 180, (len(recs), 3))
    recs["sum_a"] = np.round(base * rng.uniform(0.9, 1.1, (len(recs), 1)) * recs["n"][:, None])
    recs["sum_b"] = np.round(base * rng.uniform(0.9, 1.1, (len(recs), 1)) * recs["n"][:, None])
    cover = rng.integers(100, 900, (n, cells)).astype(np.int64)
    g = lib.solve_block_gains(recs, pairs, cover, grid_x=gx, grid_y=gy, smooth=0, channels=1)
    assert lib.solve_block_gains(recs, pairs, cover, grid_x=gx, grid_y=gy, smooth=0, channels=1).tobytes() == g.tobytes()
    ref = br.solve_ref(recs, pairs, cover, gx, gy, channels=1)
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(g.astype(np.float64) - ref) <= ulp)


def test_node_without_equation_gets_one(lib):
    dead = [(2, 5), (0, 0), (5, 11)]
    recs, pairs, cover = random_records(8, 4, 3, seed=5, dead=dead)
    g = lib.solve_block_gains(recs, pairs, cover, grid_x=4, grid_y=3, smooth=0)
    for k, c in dead:
        assert np.all(g[k].reshape(12, 3)[c] == 1.0)
    assert rel_err(g, br.solve_ref(recs, pairs, cover, 4, 3)) < 1e-7
    # records with n == 0 add nothing
    extra = recs[:3].copy(); extra["n"] = 0; extra["cell_b"] = (extra["cell_b"] + 1) % 12
    g2 = lib.solve_block_gains(np.concatenate([recs, extra]), pairs, cover, grid_x=4, grid_y=3, smooth=0)
    assert g2.tobytes() == g.tobytes()


@pytest.mark.parametrize("gx,gy", [(4, 3), (1, 5), (16, 16), (1, 1)])
@pytest.mark.parametrize("smooth", [0, 1, 2, 8])
def test_smoothing(lib, gx, gy, smooth):
    n = 3
    recs, pairs, cover = random_records(n, gx, gy, seed=smooth + 1, density=0.4)
    raw = br.solve_ref(recs, pairs, cover, gx, gy)
    g = lib.solve_block_gains(recs, pairs, cover, grid_x=gx, grid_y=gy, smooth=smooth)
    ref = br.smooth_ref(raw, smooth)
    assert rel_err(g, ref) < 1e-7
    if smooth and gx * gy > 1:
        assert np.ptp(ref) < np.ptp(raw)


def test_solve_argument_errors(lib):
    recs, pairs, cover = random_records(6, 4, 3, seed=2)

    def err(match, r=recs, p=pairs, c=cover, **kw):
        kw = dict(dict(grid_x=4, grid_y=3), **kw)
        with pytest.raises(lib.Mi355Error) as e:
            lib.solve_block_gains(r, p, c, **kw)
        assert e.value.code == -1 and match in str(e.value), str(e.value)

    bad = recs.copy(); bad[4]["pair"] = len(pairs)
    err("record 4: pair=%d outside [0, %d)" % (len(pairs), len(pairs)), r=bad)
    bad = recs.copy(); bad[1]["pair"] = -1
    err("record 1: pair=-1", r=bad)
    bad = recs.copy(); bad[2]["cell_a"] = 12
    err("record 2: cell (12, ", r=bad)
    bad = recs.copy(); bad[3]["cell_b"] = -1
    err("record 3: cell (", r=bad)
    bad = recs.copy(); bad[0]["n"] = -5
    err("record 0: n=-5 < 0", r=bad)
    badc = cover.copy(); badc[2, 7] = -1
    err("frame 2 cell 7: cell_cover=-1 < 0", c=badc)
    err("pair 1 (1, 1): a == b", p=[pairs[0], (1, 1)] + pairs[2:])
    err("position outside [0, 6)", p=[(0, 6)] + pairs[1:])
    err("repeats pair 0", p=[pairs[0], (pairs[0][1], pairs[0][0])] + pairs[2:])
    err("channels=2", channels=2)
    err("sigma_n=", sigma_n=0.0)
    err("sigma_g=", sigma_g=float("nan"))
    err("smooth=9", smooth=9)
    err("smooth=-1", smooth=-1)
    err("grid 0x3", grid_x=0)
    err("grid 4x17", grid_y=17)
    err("n=0", r=recs[:0], p=[], c=np.zeros((0, 12), np.int64))


def test_default_params(lib):
    p = lib.block_gain_params()
    assert (p.sigma_n, p.channels, p.step, p.grid_x, p.grid_y, p.smooth) == (10.0, 3, 8, 8, 6, 2) and p.sigma_g == np.float32(0.1)
    assert lib.BLOCK_GAIN_STATS.itemsize == 72 and lib.BLOCK_GAIN_STATS == br.REC


def test_apply_restatement_identities():
    """the restatement itself: a map of 1.0 is the identity, a constant map equals its Q12 product whatever the grid, weights reach the cell centres"""
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (37, 53, 3)).astype(np.uint8)
    assert np.array_equal(br.apply_ref(img, np.ones((6, 8, 3), np.float32)), img)
    half = br.apply_ref(img, np.full((3, 5, 3), 0.5, np.float32))
    assert np.array_equal(half, (img.astype(np.int64) * 2048 * 256 + (1 << 19)) >> 20)
    ramp = np.zeros((1, 2, 3), np.float32); ramp[0, 1] = 2.0
    out = br.apply_ref(np.full((1, 64, 3), 100, np.uint8), ramp)
    assert np.all(out[0, :16] == 0) and np.all(out[0, 48:] == 200) and np.all(np.diff(out[0, :, 0].astype(int)) >= 0)


def test_vignetting_ranking_on_the_restatement():
    mad = br.vignette_ranking(lambda imgs, h9s, pairs, g: [br.apply_ref(i, m) for i, m in zip(imgs, g)],
                              lambda imgs, h9s, pairs, g: [gr.apply_lut(i, k) for i, k in zip(imgs, g)])
    print("vignetting: mean |a - b| over the overlaps: block %.3f, frame %.3f, none %.3f" % tuple(mad))
    # block gains must take away a good part of what the per-frame gains leave, not a sliver of it
    assert mad[0] < 0.8 * mad[1] and mad[1] < mad[2]
