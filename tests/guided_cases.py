"""Crafted features for guided matching (tests/guided_ref.py restates the stage; tests/test_guided_ref.py shows on the CPU that the cases hold what
they claim; tests/test_gpu_guided.py installs them with SetFeatures -- no SIFT run is needed).

A case is a dict: xy_i, d_i (frame i: float32 [n, 2], uint8 [n, 128]), xy_j, d_j (frame j), G (float32 [9], image j -> image i), params (the
mi355_guided_params fields that differ from the defaults), w, h, tag, and `facts` the CPU test checks.  Deterministic: the same arguments give
the same bytes."""
import numpy as np

from tests import guided_ref as gr
from tests.match_patterns import rand_desc, ulps

F = np.float32
W, H = 1000, 750
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], F)
SHIFT = np.array([1, 0, 310.37, 0, 1, -12.61, 0, 0, 1], F)
SIMILARITY = np.array([0.98, 0.05, 250.5, -0.05, 0.98, 31.25, 0, 0, 1], F)
PROJECTIVE = np.array([1.01, 0.02, 300, -0.015, 0.99, -20, 2e-6, -3e-6, 1.0], F)
ZERO_DEN = np.array([1, 0, 0, 0, 1, 0, -0.0078125, 0, 1], F)           # the denominator is exactly 0 at x = 128
GUIDES = dict(identity=IDENTITY, shift=SHIFT, similarity=SIMILARITY, projective=PROJECTIVE)
FAR = 5000.0                                                           # where keypoints that must meet nobody lie (frame i side: FAR + 100 k)


def case(tag, xy_i, d_i, xy_j, d_j, G=IDENTITY, facts=None, **params):
    return dict(tag=tag, xy_i=np.ascontiguousarray(xy_i, F).reshape(-1, 2), d_i=np.ascontiguousarray(d_i, np.uint8).reshape(-1, 128),
                xy_j=np.ascontiguousarray(xy_j, F).reshape(-1, 2), d_j=np.ascontiguousarray(d_j, np.uint8).reshape(-1, 128),
                G=np.ascontiguousarray(G, F).reshape(9), params=params, w=W, h=H, facts=facts or {})


def ref_select(c, max_selected=400, mut=""):
    return gr.select(c["xy_i"], c["d_i"], c["xy_j"], c["d_j"], c["G"], max_selected=max_selected, mut=mut, **dict(gr.DEFAULTS, **c["params"]))


def row(*vals):
    """a descriptor row: the given leading values, zeros after them"""
    r = np.zeros(128, np.uint8)
    r[:len(vals)] = vals
    return r


def scene(seed, n_i, n_j, G=IDENTITY, true=0.6, wrong=0.2, noise=1.5, tag=None, **params):
    """frame j at random places; `true` of min(n_i, n_j) keypoints of frame i sit within `noise` px of a mapped keypoint of frame j and carry its
    descriptor with +-4 of noise, `wrong` more sit inside the radius of another mapped keypoint with a descriptor of their own; the rest lie
    anywhere.  The partners are scattered over the indices of both frames."""
    rng = np.random.default_rng(seed)
    xy_j = np.stack([rng.uniform(5, W - 5, n_j), rng.uniform(5, H - 5, n_j)], 1).astype(F)
    d_j = rand_desc(rng, n_j)
    xy_i = np.stack([rng.uniform(5, W - 5, n_i), rng.uniform(5, H - 5, n_i)], 1).astype(F)
    d_i = rand_desc(rng, n_i)
    m = min(n_i, n_j)
    n_true, n_wrong = int(true * m), int(wrong * m)
    if m > 0:
        X, Y = gr.apply_div9(G, xy_j[:, 0], xy_j[:, 1])
        usable = np.nonzero(np.isfinite(X) & np.isfinite(Y))[0]
        qs = rng.permutation(usable)[:n_true + n_wrong]
        ks = rng.permutation(n_i)[:len(qs)]
        for t, (q, k) in enumerate(zip(qs, ks)):
            ang, rad = rng.uniform(0, 2 * np.pi), rng.uniform(0, noise if t < n_true else 3.5)
            xy_i[k] = (X[q] + F(rad * np.cos(ang)), Y[q] + F(rad * np.sin(ang)))
            if t < n_true:
                d_i[k] = np.clip(d_j[q].astype(np.int32) + rng.integers(-4, 5, 128), 0, 255)
    return case(tag or "scene %d x %d" % (n_i, n_j), xy_i, d_i, xy_j, d_j, G, **params)


SIZES = (0, 1, 3, 4, 255, 256, 257, 2047, 2048)


def size_cases():
    """every size on either side against 300 keypoints, and the corners (0, 0), (2048, 2048)"""
    out = [scene(100 + n, n, 300, SHIFT) for n in SIZES] + [scene(200 + n, 300, n, SHIFT) for n in SIZES]
    return out + [scene(300, 0, 0, SHIFT), scene(301, 2048, 2048, SHIFT)]


def guide_cases():
    out = [scene(400 + k, 500, 480, G, tag="guide " + name) for k, (name, G) in enumerate(sorted(GUIDES.items()))]
    c = scene(410, 400, 400, ZERO_DEN, tag="guide zero denominator at one keypoint")
    c["xy_j"][7] = (128.0, 300.0)                           # X = Y = inf or NaN there: no candidate, whatever lies around
    out.append(c)
    base = scene(411, 300, 300, IDENTITY)
    for name, G in (("all zero", np.zeros(9, F)), ("NaN in G[2]", np.where(np.arange(9) == 2, np.nan, IDENTITY)), ("inf in G[5]", np.where(np.arange(9) == 5, np.inf, IDENTITY)),
                    ("NaN in G[8]", np.where(np.arange(9) == 8, np.nan, IDENTITY)), ("-inf in G[0]", np.where(np.arange(9) == 0, -np.inf, IDENTITY))):
        out.append(dict(base, tag="guide " + name, G=np.ascontiguousarray(G, F), facts=dict(n_sel=0)))
    return out


def _lonely(n, k0=0):
    """n keypoints of frame i that meet nobody"""
    return np.stack([FAR + 100.0 * (k0 + np.arange(n)), np.full(n, FAR)], 1).astype(F)


def radius_case():
    """q0 has its only candidate at exactly radius^2 (dx = 4, dy = 0 -> 16 == 16), q1 one float32 ulp outside; q2 at (2.4, 3.2) px: 5.76 + 10.24 in
    float32 against 16"""
    xy_j = np.array([[100, 100], [300, 100], [500, 100]], F)
    xy_i = np.array([[104, 100], [ulps(304, 1), 100], [F(500) + F(2.4), F(100) + F(3.2)]], F)
    d = rand_desc(np.random.default_rng(1), 3)
    dx, dy = xy_i[2, 0] - xy_j[2, 0], xy_i[2, 1] - xy_j[2, 1]
    third = bool(dx * dx + dy * dy <= F(16))
    return case("radius edge", xy_i, d, xy_j, d, facts=dict(ids=[(0, 0)] + ([(2, 2)] if third else [])))


def stride_case():
    """2048 x 2048 keypoints, ties only at chosen (q, k): either side of the wave (64), workgroup (1024; 256 and 512 too) and pair-of-positions (2)
    strides and the last index; everything else meets nobody"""
    rng = np.random.default_rng(2)
    n = 2048
    xy_j = np.stack([-FAR - 100.0 * np.arange(n), np.full(n, -FAR)], 1).astype(F)
    xy_i = _lonely(n)
    d_j, d_i = rand_desc(rng, n), rand_desc(rng, n)
    qk = [(0, 2047), (1, 2046), (63, 1), (64, 0), (65, 255), (255, 256), (256, 257), (257, 1023), (511, 1024), (512, 1025), (1023, 511), (1024, 512),
          (1025, 3), (2046, 63), (2047, 64)]
    for t, (q, k) in enumerate(qk):
        xy_j[q] = (50.0 + 60.0 * t, 200.0)
        xy_i[k] = (50.0 + 60.0 * t + 1.25, 200.5)
        d_i[k] = d_j[q]
    return case("lane and LDS strides", xy_i, d_i, xy_j, d_j, facts=dict(ids=sorted(qk)))


def tie_cases():
    """equal d at two k (the lower k is kept; ratio 0 so that d1 == d2 does not veto it) and equal d1 from two q onto one k (the lower q keeps it)"""
    rng = np.random.default_rng(3)
    d = rand_desc(rng, 4)
    a = case("equal d at two k", [[101, 100], [99, 100], [400, 400]], [d[0], d[0], d[1]], [[100, 100], [400, 401]], [d[0], d[1]], ratio=0.0,
             facts=dict(ids=[(0, 0), (1, 2)]))
    b = case("equal d1 from two q onto one k", [[100, 100], [400, 400]], [d[0], d[1]], [[700, 700], [101, 100], [99, 101], [400, 401]], [d[3], d[0], d[0], d[1]],
             facts=dict(ids=[(1, 0), (3, 1)]))
    return [a, b]


def max_dist_cases():
    """d1 == max_dist2 (kept) and d1 == max_dist2 + 1 (not): 255^2 + 158^2 + 3^2 + 1 + 1 = 90000"""
    z = row()
    return [case("d1 == max_dist2", [[100, 100]], [row(255, 158, 3, 1, 1)], [[100, 101]], [z], facts=dict(ids=[(0, 0)], d1=[90000])),
            case("d1 == max_dist2 + 1", [[100, 100]], [row(255, 158, 3, 1, 1, 1)], [[100, 101]], [z], facts=dict(ids=[])),
            case("all 0 against all 255", [[100, 100]], [np.full(128, 255, np.uint8)], [[100, 101]], [z], max_dist2=8323200, facts=dict(ids=[(0, 0)], d1=[8323200])),
            case("max_dist2 0, equal rows", [[100, 100], [300, 300]], [row(9), row(7)], [[100, 101], [300, 301]], [row(9), row(8)], max_dist2=0, facts=dict(ids=[(0, 0)], d1=[0]))]


def ratio_cases():
    """ratio 0.5 (0.25 exactly): d1 = 100 against d2 = 400 is equality and fails, against 401 passes; ratio 0 switches the test off; one candidate
    is never tested"""
    z = row()
    two = lambda tag, second, **kw: case(tag, [[100, 100], [102, 100]], [row(10), second], [[101, 100]], [z], **kw)        # noqa: E731
    return [two("ratio at equality", row(20), ratio=0.5, facts=dict(ids=[])),
            two("ratio just passed", row(20, 1), ratio=0.5, facts=dict(ids=[(0, 0)], d1=[100])),
            two("ratio 0", row(10), ratio=0.0, facts=dict(ids=[(0, 0)], d1=[100])),
            two("ratio 1, d1 == d2", row(10), ratio=1.0, facts=dict(ids=[])),
            case("single candidate", [[100, 100]], [row(10)], [[101, 100]], [z], ratio=0.5, facts=dict(ids=[(0, 0)], d1=[100]))]


def survivor_case(n, equal_from=390, tag=None):
    """n survivors, each q its own k (k = n - 1 - q: the orders by q and by k differ); d1 = q for q < equal_from and d1 = equal_from for the rest, so
    the cut at 400 falls inside a run of equal d1 and only (d1, q) decides who stays"""
    xy_j = np.stack([20.0 + 17.0 * (np.arange(n) % 50), 20.0 + 17.0 * (np.arange(n) // 50)], 1).astype(F)
    xy_i = (xy_j + F(0.5))[::-1].copy()
    d_j = np.zeros((n, 128), np.uint8)
    d_i = np.zeros((n, 128), np.uint8)
    for q in range(n):
        v = min(q, equal_from)
        d_i[n - 1 - q, :v] = 1                              # d1 = v ones
    want = [(q, n - 1 - q) for q in range(min(n, 400))]
    return case(tag or "%d survivors" % n, xy_i, d_i, xy_j, d_j, facts=dict(ids_in_order=want, n_survivors=n))


def cut_cases():
    return [survivor_case(401), survivor_case(500), survivor_case(3, tag="n_sel 3"), survivor_case(4, tag="n_sel 4"), survivor_case(400)]


def planted_case(seed=7, n_true=300, n_wrong=100, n_other=600):
    """a planar pair: n_true keypoints of frame j with their partners in frame i (0.5 px of noise, the descriptor with +-3) and n_wrong more whose only
    neighbour inside the radius is a stranger that happens to look alike (descriptor +-12: under max_dist2), all under PROJECTIVE"""
    rng = np.random.default_rng(seed)
    n = n_true + n_wrong
    xy_j = np.stack([rng.uniform(40, W - 40, n + n_other), rng.uniform(40, H - 40, n + n_other)], 1).astype(F)
    d_j = rand_desc(rng, n + n_other)
    X, Y = gr.apply_div9(PROJECTIVE, xy_j[:n, 0], xy_j[:n, 1])
    xy_i = np.zeros((n + n_other, 2), F)
    d_i = rand_desc(rng, n + n_other)
    xy_i[n:] = np.stack([rng.uniform(-3000, -100, n_other), rng.uniform(-3000, -100, n_other)], 1)
    xy_i[:n_true] = np.stack([X[:n_true] + rng.normal(0, 0.5, n_true), Y[:n_true] + rng.normal(0, 0.5, n_true)], 1)
    ang = rng.uniform(0, 2 * np.pi, n_wrong)
    xy_i[n_true:n] = np.stack([X[n_true:] + 3.5 * np.cos(ang), Y[n_true:] + 3.5 * np.sin(ang)], 1)
    d_i[:n_true] = np.clip(d_j[:n_true].astype(np.int32) + rng.integers(-3, 4, (n_true, 128)), 0, 255)
    d_i[n_true:n] = np.clip(d_j[n_true:n].astype(np.int32) + rng.integers(-12, 13, (n_wrong, 128)), 0, 255)
    perm_i, perm_j = rng.permutation(n + n_other), rng.permutation(n + n_other)
    return case("planted planar pair", xy_i[perm_i], d_i[perm_i], xy_j[perm_j], d_j[perm_j], PROJECTIVE, facts=dict(n_true=n_true, n_wrong=n_wrong))


def crafted_cases():
    """the small cases whose outcome is stated in `facts`"""
    return [radius_case(), stride_case()] + tie_cases() + max_dist_cases() + ratio_cases() + cut_cases()


def all_cases():
    return crafted_cases() + size_cases() + guide_cases() + [planted_case()]
