"""numpy restatement of cover depth (include/mi355_mosaic.h, "cover depth"; csrc/cover.hip, csrc/cover_select.cpp), written from the header.

Cover is the gain stage's: the per-frame cover maps gain_ref.frame_sample_maps makes from the oracle's refined render (maps[k][1]), on
gain_ref.lattice.  geometry() restates the same maps, and the frames' clipped canvas boxes the selection needs, without the oracle, through
tests/warp_ref.py (the refined render's map, as block_gain_ref.coord_maps does): it serves layouts of hundreds of frames, for which one oracle
render per frame is too slow, and the mutation "cover without the box test".  tests/test_cover_patterns_ref.py holds the two together.

stats_ref gives the integers; select_rounds is the round rule of the header; select_sequential is the plain greedy that recomputes the
statistics after every single drop.
"""
import numpy as np

from tests import gain_ref as gr
from tests import warp_ref as wr

f32 = np.float32
BINS = 9
FRAME_STATS = np.dtype([("at_depth", "<i8", (8,))])
NOT_CANDIDATE, DROPPED, KEPT_COVERAGE, CUT_VERTEX, NOT_EXAMINED = 0, 1, 2, 3, 4


# ---- geometry ---------------------------------------------------------------------------------------------------------------------------------
def geometry(sizes, h9s, eps=1e-12, box_test=True, want_covers=True):
    """sizes: [(w, h)].  (covers, boxes, (cw, ch)): per frame None where it takes no part, else its cover [ch, cw] bool and its clipped canvas
    box (x0, x1, y0, y1), ends included.  box_test=False: the map's bounds test alone, over the whole canvas (a mutation)."""
    n = len(sizes)
    h9s = np.asarray(h9s, np.float32).reshape(n, 9)
    live = [k for k in range(n) if h9s[k, 8] != 0]
    minX, minY, maxX, maxY = wr.BIG, wr.BIG, -wr.BIG, -wr.BIG
    proj = {}
    for k in live:
        X, Y = wr.project(h9s[k], *wr.corners(*sizes[k]))
        proj[k] = (X, Y)
        for x, y in zip(X, Y):
            if x < minX: minX = x
            if x > maxX: maxX = x
            if y < minY: minY = y
            if y > maxY: maxY = y
    cw, ch = wr._extent(minX, maxX), wr._extent(minY, maxY)
    dGX, dGY = -minX, -minY
    covers, boxes = [None] * n, [None] * n
    for k in live:
        inv = wr.inverse(h9s[k], eps)
        if inv is None:
            continue
        X, Y = proj[k]
        X = X + (f32(0) + dGX); Y = Y + (f32(0) + dGY)
        bminX, bminY, bmaxX, bmaxY = wr._box(X, Y)
        x0, x1 = max(int(f32(bminX - f32(0.5))), 0), min(int(f32(bmaxX + f32(0.5))), cw - 1)
        y0, y1 = max(int(f32(bminY - f32(0.5))), 0), min(int(f32(bmaxY + f32(0.5))), ch - 1)
        if x1 < x0 or y1 < y0:
            continue
        boxes[k] = (x0, x1, y0, y1)
        if not want_covers:
            covers[k] = True
            continue
        bx0, bx1, by0, by1 = (x0, x1, y0, y1) if box_test else (0, cw - 1, 0, ch - 1)
        xf = (np.arange(bx0, bx1 + 1).astype(np.float32) - dGX)[None, :].repeat(by1 - by0 + 1, 0)
        yf = (np.arange(by0, by1 + 1).astype(np.float32) - dGY)[:, None].repeat(bx1 - bx0 + 1, 1)
        xs, ys = wr.project(inv, xf, yf)
        c = np.zeros((ch, cw), bool)
        c[by0:by1 + 1, bx0:bx1 + 1] = wr._has_sample(xs, ys, *sizes[k])
        covers[k] = c
    return covers, boxes, (cw, ch)


def covers_of(maps):
    """the cover maps of gain_ref.frame_sample_maps' result"""
    return [None if m is None else m[1] for m in maps]


def kept_of(covers, keep):
    """the kept frames: those that take part and have keep[k] != 0 (keep None: every frame)"""
    return [c is not None and (keep is None or bool(keep[k])) for k, c in enumerate(covers)]


# ---- statistics -------------------------------------------------------------------------------------------------------------------------------
def depth_map(covers, keep, shape):
    d = np.zeros(shape, np.int64)
    for c, kp in zip(covers, kept_of(covers, keep)):
        if kp:
            d += c
    return d


def stats_ref(covers, keep, step, shape, saturate=8):
    """(FRAME_STATS [n], hist int64 [BINS]) under keep on the lattice of `step` of the [ch, cw] canvas.  saturate: the depth at which the last
    bucket begins (8; anything else is a mutation)"""
    L = gr.lattice(shape[0], shape[1], step)
    d = depth_map(covers, keep, shape)
    b = np.minimum(d, saturate)
    hist = np.bincount(b[L], minlength=BINS).astype(np.int64)[:BINS]
    fs = np.zeros(len(covers), FRAME_STATS)
    for k, kp in enumerate(kept_of(covers, keep)):
        if kp:
            fs["at_depth"][k] = np.bincount(b[covers[k] & L] - 1, minlength=8)[:8]
    return fs, hist


def crit(fs, k, min_depth, inclusive=True):
    """the lattice points of k with depth <= min_depth (inclusive=False: < min_depth, a mutation)"""
    return int(fs["at_depth"][k][:min_depth if inclusive else min_depth - 1].sum())


# ---- selection --------------------------------------------------------------------------------------------------------------------------------
def _meets(a, b):
    return a[0] <= b[1] and b[0] <= a[1] and a[2] <= b[3] and b[2] <= a[3]


def _adjacency(n, pairs, kept):
    adj = [[] for _ in range(n)]
    for a, b in (pairs if pairs is not None else ()):
        if kept[a] and kept[b]:
            adj[a].append(b); adj[b].append(a)
    return adj


def _reach(adj, kept, start, without):
    seen, stack = {start}, [start]
    while stack:
        for q in adj[stack.pop()]:
            if q != without and kept[q] and q not in seen:
                seen.add(q); stack.append(q)
    return seen


def stays_connected(adj, kept, k):
    """the still-kept frames of k's component stay connected without k (none left: nothing to split)"""
    others = _reach(adj, kept, k, None) - {k}
    if not others:
        return True
    return _reach(adj, kept, next(iter(sorted(others))), k) == others


def _candidates(n, part, keep, order):
    kept = [bool(part[k]) and (keep is None or bool(keep[k])) for k in range(n)]
    status = np.zeros(n, np.uint8)
    if order is None:
        return kept, status, [k for k in range(n) if kept[k]]
    assert len(set(order)) == len(order)
    for k in order:
        if not kept[k]:
            status[k] = NOT_EXAMINED
    return kept, status, [k for k in order if kept[k]]


def select_rounds(n, boxes, stats_fn, order=None, pairs=None, keep=None, min_depth=1, max_loss=0, inclusive=True, block_waiting=True):
    """the round rule.  boxes[k]: None where k takes no part; stats_fn(keep uint8 [n]) -> FRAME_STATS [n].  Returns (status, keep_out, rounds,
    lost).  inclusive / block_waiting = False are mutations (crit over d < min_depth; blocked boxes omit the waiting candidates)."""
    kept, status, waiting = _candidates(n, [b is not None for b in boxes], keep, order)
    adj = _adjacency(n, pairs, list(kept))
    rounds, lost = 0, 0
    while waiting:
        fs = stats_fn(np.array(kept, np.uint8))
        rounds += 1
        if order is None and rounds == 1:
            waiting.sort(key=lambda k: (crit(fs, k, min_depth, inclusive), k))
        blocked, nxt = [], []
        for k in waiting:
            if any(_meets(boxes[k], b) for b in blocked):
                nxt.append(k)
                if block_waiting:
                    blocked.append(boxes[k])
                continue
            c = crit(fs, k, min_depth, inclusive)
            if c > max_loss:
                status[k] = KEPT_COVERAGE
            elif pairs is not None and len(pairs) and not stays_connected(adj, kept, k):
                status[k] = CUT_VERTEX
            else:
                status[k], kept[k] = DROPPED, False
                lost += c
                blocked.append(boxes[k])
        waiting = nxt
    return status, np.array(kept, np.uint8), rounds, lost


def select_sequential(n, boxes, stats_fn, order=None, pairs=None, keep=None, min_depth=1, max_loss=0):
    """the plain greedy: the candidates once, in order, the statistics taken again after every single drop.  (status, keep_out, lost)"""
    kept, status, cands = _candidates(n, [b is not None for b in boxes], keep, order)
    adj = _adjacency(n, pairs, list(kept))
    lost = 0
    fs = stats_fn(np.array(kept, np.uint8)) if cands else None
    if order is None and cands:
        cands.sort(key=lambda k: (crit(fs, k, min_depth), k))
    for k in cands:
        c = crit(fs, k, min_depth)
        if c > max_loss:
            status[k] = KEPT_COVERAGE
        elif pairs is not None and len(pairs) and not stays_connected(adj, kept, k):
            status[k] = CUT_VERTEX
        else:
            status[k], kept[k] = DROPPED, False
            lost += c
            fs = stats_fn(np.array(kept, np.uint8))
    return status, np.array(kept, np.uint8), lost
