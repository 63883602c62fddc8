"""The later stages on ONE used context: the step tables, the runner and the CPU-side facts about each table.

Every call takes its device and pinned workspaces from the context's named, grow-only buffers (csrc/common.h: ctx->buf, ctx->hbuf).  A buffer
is never cleared when it is reused, so a call that follows a larger one finds that call's bytes in every workspace it does not fully write;
a fresh context in a fresh process cannot show a missing clear or an unwritten tail, because a new allocation comes back zeroed (later
in a process it may hold freed bytes: with a clear taken out, fresh contexts went wrong as well).  The suites of the stages run each on a
fresh context.  The tables here run them interleaved on one, large cases before small ones and stages that share buffers next to
each other, and every step is held to

  1. its stage's own reference (the numpy restatement or the oracle its suite uses), byte for byte, and
  2. the bytes of the same call on a fresh context -- which also says, when 1. fails, whether reuse is the cause.

A Step knows, besides its call and its reference, what it leaves in each shared buffer it writes (`leaves`: buffer -> number of entries, from
the case's own numbers).  tests/test_used_context_plan.py asserts on a CPU-only machine that for every shared buffer some step comes after
one that left MORE there than the step itself writes, that the two steps' references differ, and that every reference is computable.  The
tables: render_steps (tests/test_gpu_used_context_renders.py), chip_steps (.._chips.py), pair_steps (.._pairs.py).

Nothing here poisons a workspace: the stale bytes are those of a larger earlier call, which stay inside the allocations.
"""
from typing import Callable, NamedTuple, Optional

import numpy as np

FILL8, FILL16, TAIL = 7, 0x5555, 201                                        # device canvases, device maps, host rows before a call
WIDER = 8                                                                   # a caller's row is this much wider than the layout's


class Step(NamedTuple):
    name: str
    run: Callable                       # run(env, ctx) -> list of numpy arrays
    ref: Optional[Callable]             # ref(orc) -> list as run's, an entry None where only the fresh context is the yardstick
    leaves: dict                        # shared buffer -> entries this step writes there
    case: str = ""                      # the survey or record set the step runs on


class Env:
    """what the calls need on the GPU machine: torch, the package, and the uploads made so far (one per key)"""

    def __init__(self, torch, im):
        self.torch, self.im, self.held = torch, im, {}

    def once(self, key, make):
        if key not in self.held:
            self.held[key] = make()
        return self.held[key]

    def full(self, shape, fill, dtype):
        t = self.torch.full(shape, fill, dtype=dtype, device="cuda")
        self.torch.cuda.synchronize()                                       # the fill runs on torch's stream, the library on the ctx's own
        return t

    def dev(self, a):
        t = self.torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
        self.torch.cuda.synchronize()
        return t

    def upload(self, imgs, pad=5, fill=0xEE):
        """device copies [h, 3 w + pad] of host images, the padding poisoned: (tensors, ptrs, w, h, ws)"""
        ts = []
        for a in imgs:
            h, w = a.shape[:2]
            b = np.full((h, 3 * w + pad), fill, np.uint8)
            b[:, :3 * w] = a.reshape(h, 3 * w)
            ts.append(self.torch.from_numpy(b).cuda())
        self.torch.cuda.synchronize()
        return ts, [t.data_ptr() for t in ts], [a.shape[1] for a in imgs], [a.shape[0] for a in imgs], [t.shape[1] for t in ts]


# ---- the runner -----------------------------------------------------------------------------------------------------------------------------------
def as_array(v):
    """results as arrays: a report dict by its sorted items, a structured array by its bytes"""
    if isinstance(v, dict):
        return np.array([int(v[k]) for k in sorted(v)], np.int64)
    a = np.asarray(v)
    if a.dtype.fields is not None:
        a = np.ascontiguousarray(a).view(np.uint8).reshape(a.shape + (a.dtype.itemsize,))
    return a


def first_difference(got, want):
    """None, or a sentence on the first output that differs: which, how many values, the first differing indices"""
    if len(got) != len(want):
        return "%d outputs against %d" % (len(got), len(want))
    for i, (a, b) in enumerate(zip(got, want)):
        if b is None:
            continue
        a, b = as_array(a), as_array(b)
        if a.shape != b.shape:
            return "output %d: shape %s against %s" % (i, a.shape, b.shape)
        bad = a != b
        if bad.any():
            return "output %d: %d of %d values differ, first at %s" % (i, int(bad.sum()), bad.size, np.argwhere(bad)[:5].tolist())
    return None


def run_steps(env, steps, orc):
    """all steps on one context, then each on a fresh one; every step against its reference and against the fresh context.  Returns
    {name: outputs on the used context}; raises AssertionError naming every step that differs, with the first differing indices.  A call the
    library refuses (Mi355Error: stale sums can make one) counts as a difference of that step and the others still run."""
    im = env.im
    assert len({s.name for s in steps}) == len(steps)

    def outputs(s, ctx):
        try:
            return [as_array(v) for v in s.run(env, ctx)]
        except im.Mi355Error as e:
            return e
    ctx = im.Context(0)
    used = [outputs(s, ctx) for s in steps]
    ctx.close()
    problems = []
    for s, got in zip(steps, used):
        fresh = im.Context(0)
        alone = outputs(s, fresh)
        fresh.close()
        if isinstance(got, Exception) or isinstance(alone, Exception):
            problems.append("%s: refused on %s: %s" % (s.name, " and ".join(w for w, v in (("the used context", got), ("a fresh one", alone)) if isinstance(v, Exception)),
                                                     got if isinstance(got, Exception) else alone))
            continue
        assert len(got) > 0, s.name
        want = s.ref(orc) if s.ref is not None else [None] * len(got)
        d_ref, d_fresh, d_alone = first_difference(got, want), first_difference(got, alone), first_difference(alone, want)
        if d_ref and not d_alone:
            problems.append("%s: REUSE: differs from its reference on the used context only (%s)" % (s.name, d_ref))
        elif d_ref:
            problems.append("%s: differs from its reference on the used context (%s) and on a fresh one (%s)" % (s.name, d_ref, d_alone))
        if d_fresh:
            problems.append("%s: differs from the same call on a fresh context (%s)" % (s.name, d_fresh))
    assert not problems, "\n".join(problems)
    return dict(zip([s.name for s in steps], used))


# ---- the CPU-side facts ---------------------------------------------------------------------------------------------------------------------------
def leak_chances(steps, buffer):
    """[(later step, earlier step)]: the later step writes fewer entries of `buffer` than the earlier one left there.  The bytes just past what
    the later step writes are those of the LAST earlier step that wrote more, so that one is the partner."""
    out = []
    for i, s in enumerate(steps):
        if buffer not in s.leaves:
            continue
        for j in range(i - 1, -1, -1):
            if steps[j].leaves.get(buffer, 0) > s.leaves[buffer]:
                out.append((i, j))
                break
    return out


def references_differ(a, b):
    """two steps' references differ in content: some output of one has no equal among the other's (another shape is another content)"""
    a, b = [as_array(v) for v in a if v is not None], [as_array(v) for v in b if v is not None]
    return any(not any(x.shape == y.shape and np.array_equal(x, y) for y in b) for x in a)


def buffers_of(steps):
    return sorted({b for s in steps for b in s.leaves})


# ==== the frame-table family: renders, covers, gains, overviews ====================================================================================
LIST_BLOCK = 256                                                            # csrc/mosaic_frame.h: MOSAIC_LIST_BLOCK
# (seamcut_energy is three accumulators whatever the grid: no call writes fewer; every step that reports energies reads all three)
RENDER_SHARED = ("mosaic_frames", "feather_ramps", "seamline_frame_of", "mosaic_lists", "mosaic_counts", "mosaic_used", "seamline_owner",
                 "seamcut_labels", "seamcut_sums", "seamcut_candidates", "seamcut_cells", "median_spread", "gain_frames", "gain_acc",
                 "gain_tiles", "block_gain_acc", "block_gain_cover", "gain_apply_frames", "block_gain_apply_frames", "into_srcs", "into_canvas",
                 "mosaic_srcs", "mosaic_canvas", "download", "overview_canvas", "preview_stripe")
_SURVEYS = {}


class Survey:
    """a survey under integer translations whose smallest offset is (0, 0) -- the canvas and every frame's rows follow from the offsets alone --
    with the references every render step needs, each computed once and not to be written to"""

    def __init__(self, name, imgs, h9s, p, pairs):
        self.name, self.imgs, self.h9s, self.p, self.pairs = name, [np.ascontiguousarray(a) for a in imgs], np.asarray(h9s, np.float32), dict(p), list(pairs)
        self.n = len(imgs)
        t = self.h9s.reshape(self.n, 3, 3)
        assert np.array_equal(t[:, :2, :2], np.tile(np.eye(2, dtype=np.float32), (self.n, 1, 1))) and np.all(t[:, 2] == [0, 0, 1])
        self.offs = [(int(t[k, 0, 2]), int(t[k, 1, 2])) for k in range(self.n)]
        assert all(t[k, 0, 2] == ox and t[k, 1, 2] == oy for k, (ox, oy) in enumerate(self.offs)) and min(o[0] for o in self.offs) == 0 == min(o[1] for o in self.offs)
        self.w, self.h = [a.shape[1] for a in self.imgs], [a.shape[0] for a in self.imgs]
        self.cw = max(ox + w for (ox, oy), w in zip(self.offs, self.w))
        self.ch = max(oy + h for (ox, oy), h in zip(self.offs, self.h))
        self.lws = (3 * self.cw + 3) & ~3
        self.cws = self.lws + WIDER
        self._c = {}

    # -- the case's own numbers
    def frames_in(self, row0=0, rows=None):
        """the frames whose box meets canvas rows [row0, row0 + rows): the entries of the frame table"""
        row1 = self.ch if rows is None else row0 + rows
        return sum(1 for (ox, oy), h in zip(self.offs, self.h) if oy < row1 and oy + h - 1 >= row0)

    def blocks(self, rows=None):
        return -(-self.cw // LIST_BLOCK) * -(-(self.ch if rows is None else rows) // LIST_BLOCK)

    def grid(self, level=None):
        s = 1 << (self.p["level"] if level is None else level)
        return -(-self.cw // s), -(-self.ch // s)

    def table(self, ramps, frame_of, row0=0, rows=None, used=False):
        """what a frame-table upload over these rows leaves"""
        nf, b = self.frames_in(row0, rows), self.blocks(rows)
        d = {"mosaic_frames": nf, "mosaic_lists": nf * b, "mosaic_counts": b}
        if ramps:
            d["feather_ramps"] = nf
        if frame_of:
            d["seamline_frame_of"] = nf
        if used:
            d["mosaic_used"] = nf
        return d

    def src_bytes(self):
        return sum(3 * w * h for w, h in zip(self.w, self.h))

    # -- references
    def _once(self, key, make):
        if key not in self._c:
            self._c[key] = make()
        return self._c[key]

    def maps(self, orc):
        from tests import gain_ref as gr
        m = self._once("maps", lambda: gr.frame_sample_maps(orc, self.imgs, self.h9s))
        assert next(x for x in m if x is not None)[1].shape == (self.ch, self.cw)
        return m

    def wmaps(self, orc, ramp=0):
        from tests import seamline_ref as sr
        return self._once(("wmaps", ramp), lambda: sr.weight_maps(orc, self.imgs, self.h9s, ramp, self.maps(orc)))

    def rows_of(self, pix, cws=None, fill=0):
        """[ch, cw, 3] reference pixels as the rows of a device canvas: [ch, cws] with the padding zeroed (or left at `fill`)"""
        out = np.full((pix.shape[0], self.cws if cws is None else cws), fill, np.uint8)
        out[:, :3 * self.cw] = pix.reshape(pix.shape[0], 3 * self.cw)
        return out

    def median(self, orc, depth, ramp=0):
        from tests import median_ref as mr
        return self._once(("median", depth, ramp), lambda: mr.pick(self.maps(orc), self.wmaps(orc, ramp), depth))

    def seamline(self, orc, ramp=0):
        from tests import seamline_ref as sr
        return self._once(("seamline", ramp), lambda: sr.pick(self.maps(orc), self.wmaps(orc, ramp))[:3])

    def feathered(self, orc, ramp):
        from tests import feather_ref as fr
        return self._once(("feather", ramp), lambda: fr.blend(self.maps(orc), self.wmaps(orc, ramp))[0])

    def refined(self, orc):
        def make():
            rc, r = orc.mosaic_images_refined(self.imgs, self.h9s)
            assert rc == 0 and (r[1], r[2]) == (self.cw, self.ch)
            return np.ascontiguousarray(r[0][:, :3 * self.cw]).reshape(self.ch, self.cw, 3)
        return self._once("refined", make)

    def seamcut(self, orc):
        from tests import seamcut_ref as sc
        return self._once("seamcut", lambda: sc.seamcut_ref(orc, self.imgs, self.h9s, self.p, maps=self.maps(orc), wmaps=self.wmaps(orc, self.p["ramp"])))


def render_surveys():
    """L  tests/blend_seam_patterns.big: twelve 128 x 96 frames, a canvas wider and higher than 256 px (four list blocks), cells at level 3
       W  tests/seamcut_patterns.py wave130: 130 frames of 12 .. 16 px a side on a 24 x 24 canvas (one list block, 130 table entries)
       S  tests/seamcut_patterns.crafted(frames=2): two 64 x 96 frames, cells at level 2
       B  the 32 x 24 two-frame survey of tests/test_gpu_render_interleave.py: canvas rows 24 .. 98 meet no frame's box"""
    if "L" not in _SURVEYS:
        from tests import blend_seam_patterns as bp
        from tests import seamcut_patterns as sp
        from tests import seamcut_ref as sc
        from tests.test_gpu_render_interleave import _survey_b
        big = bp.big()
        near = lambda S_offs, w, h: [(a, b) for a in range(len(S_offs)) for b in range(a + 1, len(S_offs))
                                     if abs(S_offs[a][0] - S_offs[b][0]) < w - 2 and abs(S_offs[a][1] - S_offs[b][1]) < h - 2]
        L = Survey("L", big.imgs, big.h9s, sc.params(level=3, depth=8), [])
        L.pairs = near(L.offs, 128, 96) + [(0, 11)]                         # the last pair has no overlap
        wi, wh, wp = sp.WAVE_CASES["wave130"]()
        W = Survey("W", wi, wh, wp, [])
        W.pairs = [(k, (k * 7 + 3) % 130) for k in range(130) if k != (k * 7 + 3) % 130][:120]
        W.pairs = sorted({(min(a, b), max(a, b)) for a, b in W.pairs})
        si, sh, sp_ = sp.crafted(2)[:3]
        S = Survey("S", si, sh, sp_, [(0, 1)])
        bi, bh, _ = _survey_b()
        B = Survey("B", bi, bh, sc.params(level=2), [(0, 1)])
        _SURVEYS.update(L=L, W=W, S=S, B=B)
    return _SURVEYS


def _devs(env, S):
    return env.once(("frames", S.name), lambda: env.upload(S.imgs))


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


def _layout_ok(env, S, up):
    cw, ch, lws, _ = env.im.mosaic_layout(up[2], up[3], S.h9s)
    assert (cw, ch, lws) == (S.cw, S.ch, S.lws), (S.name, cw, ch, lws)


def _median(S, depth, ramp=0):
    def run(env, ctx):
        torch = env.torch
        up = _devs(env, S)
        _layout_ok(env, S, up)
        c = env.full((S.ch, S.cws), FILL8, torch.uint8)
        spread = env.full((S.ch, S.cw), 0x33, torch.uint8)
        count = env.full((S.ch, S.cw), FILL16, torch.int16)
        ctx.MosaicMedianDev(up[1], up[2], up[3], up[4], S.h9s, c.data_ptr(), S.cw, S.ch, S.cws, d_spread=spread.data_ptr(), d_count=count.data_ptr(), ramp=ramp, depth=depth)
        return [c.cpu().numpy(), spread.cpu().numpy(), _u16(count)]

    def ref(orc):
        out, spread, count = S.median(orc, depth, ramp)[:3]
        return [S.rows_of(out), spread, count]
    return Step("median %s, depth %d" % (S.name, depth), run, ref, S.table(True, False), S.name)


def _seamline(S, canvas=True):
    def run(env, ctx):
        torch = env.torch
        up = _devs(env, S)
        _layout_ok(env, S, up)
        c = env.full((S.ch, S.cws), FILL8, torch.uint8) if canvas else None
        own, cnt = env.full((S.ch, S.cw), FILL16, torch.int16), env.full((S.ch, S.cw), FILL16, torch.int16)
        if canvas:
            ctx.MosaicSeamlineDev(up[1], up[2], up[3], up[4], S.h9s, c.data_ptr(), S.cw, S.ch, S.cws, d_owner=own.data_ptr(), d_count=cnt.data_ptr())
        else:
            ctx.MosaicSeamlineDev(None, up[2], up[3], None, S.h9s, 0, S.cw, S.ch, S.cws, d_owner=own.data_ptr(), d_count=cnt.data_ptr())
        return ([c.cpu().numpy()] if canvas else []) + [_u16(own), _u16(cnt)]

    def ref(orc):
        out, owner, count = S.seamline(orc)
        return ([S.rows_of(out)] if canvas else []) + [owner, count]
    return Step("seamline %s%s" % (S.name, "" if canvas else ", maps only"), run, ref, S.table(True, True), S.name)


def _seamline_host(S):
    """the host form keeps the owner map in the ctx's own seamline_owner"""
    def run(env, ctx):
        r = ctx.MosaicSeamline(S.imgs, S.h9s, want_owner=True)
        return [r[0], r[4]]

    def ref(orc):
        out, owner, _ = S.seamline(orc)
        return [S.rows_of(out, S.lws), owner]
    return Step("seamline host %s" % S.name, run, ref, dict(S.table(True, True), seamline_owner=S.cw * S.ch, mosaic_srcs=S.src_bytes(), mosaic_canvas=S.ch * S.lws,
                                                          download=S.ch * S.lws), S.name)


def _seamcut(S, one_call):
    """one_call: candidates, labels and render inside MosaicSeamCutDev (the ctx's own record and cell buffers); else the three entry points, the
    records, the cell map and the report compared as well"""
    gw, gh = S.grid()
    cells = gw * gh

    def run(env, ctx):
        torch = env.torch
        up = _devs(env, S)
        _layout_ok(env, S, up)
        out = []
        d_cells = 0
        if not one_call:
            assert env.im.seam_grid(up[2], up[3], S.h9s, S.p["level"]) == (gw, gh)
            d_cand = env.full((cells * 32,), 0xAB, torch.uint8)
            t_cells = env.full((cells,), 0x7777, torch.int16)
            ctx.SeamCandidatesDev(up[1], up[2], up[3], up[4], S.h9s, d_cand.data_ptr(), gw, gh, **S.p)
            rep = ctx.SeamLabelsDev(d_cand.data_ptr(), gw, gh, t_cells.data_ptr(), **S.p)
            t2 = env.full((cells,), 0x1111, torch.int16)
            rep2 = ctx.SeamCellsDev(up[1], up[2], up[3], up[4], S.h9s, t2.data_ptr(), gw, gh, **S.p)
            out += [d_cand.cpu().numpy().reshape(gh, gw, 32), _u16(t_cells).reshape(gh, gw), rep, _u16(t2).reshape(gh, gw), rep2]
            d_cells = t_cells.data_ptr()
        c = env.full((S.ch, S.cws), FILL8, torch.uint8)
        own, cnt = env.full((S.ch, S.cw), FILL16, torch.int16), env.full((S.ch, S.cw), FILL16, torch.int16)
        ctx.MosaicSeamCutDev(up[1], up[2], up[3], up[4], S.h9s, c.data_ptr(), S.cw, S.ch, S.cws, d_cells=d_cells, d_owner=own.data_ptr(), d_count=cnt.data_ptr(), **S.p)
        return out + [c.cpu().numpy(), _u16(own), _u16(cnt)]

    def ref(orc):
        r = S.seamcut(orc)
        head = [] if one_call else [r["records"], r["cells"], r["report"], r["cells"], r["report"]]
        return head + [S.rows_of(r["canvas"]), r["owner"], r["count"]]
    leaves = dict(S.table(True, True), seamcut_labels=cells, seamcut_sums=8 * cells, seamcut_energy=3)
    if one_call:
        leaves.update(seamcut_candidates=cells, seamcut_cells=cells)
    return Step("seamcut %s, %s" % (S.name, "one call" if one_call else "three stages"), run, ref, leaves, S.name)


def _seamcut_forms(S, form):
    """the host form (owner map in the ctx's seamline_owner) and the _into form"""
    gw, gh = S.grid()
    cells = gw * gh

    def run(env, ctx):
        if form == "host":
            r = ctx.MosaicSeamCut(S.imgs, S.h9s, want_owner=True, **S.p)
            return [r[0], r[4]]
        out = np.full((S.ch, 3 * S.cw + 13), TAIL, np.uint8)
        ctx.MosaicSeamCutInto(S.imgs, None, S.h9s, out=out, **S.p)
        return [out]

    def ref(orc):
        r = S.seamcut(orc)
        return [S.rows_of(r["canvas"], S.lws), r["owner"]] if form == "host" else [S.rows_of(r["canvas"], 3 * S.cw + 13, TAIL)]
    leaves = dict(S.table(True, True), seamcut_labels=cells, seamcut_sums=8 * cells, seamcut_energy=3, seamcut_candidates=cells, seamcut_cells=cells, download=S.ch * S.lws)
    leaves.update(dict(seamline_owner=S.cw * S.ch, mosaic_srcs=S.src_bytes(), mosaic_canvas=S.ch * S.lws) if form == "host" else
                  dict(into_srcs=S.src_bytes(), into_canvas=S.ch * S.lws))
    return Step("seamcut %s %s" % (form, S.name), run, ref, leaves, S.name)


def _median_forms(S, form, depth):
    def run(env, ctx):
        if form == "host":
            r = ctx.MosaicMedian(S.imgs, S.h9s, depth=depth, want_spread=True)
            return [r[0], r[4]]
        out = np.full((S.ch, 3 * S.cw + 13), TAIL, np.uint8)
        ctx.MosaicMedianInto(S.imgs, None, S.h9s, out=out, depth=depth)
        return [out]

    def ref(orc):
        out, spread = S.median(orc, depth)[:2]
        return [S.rows_of(out, S.lws), spread] if form == "host" else [S.rows_of(out, 3 * S.cw + 13, TAIL)]
    leaves = dict(S.table(True, False), download=S.ch * S.lws)
    leaves.update(dict(median_spread=S.cw * S.ch, mosaic_srcs=S.src_bytes(), mosaic_canvas=S.ch * S.lws) if form == "host" else
                  dict(into_srcs=S.src_bytes(), into_canvas=S.ch * S.lws))
    return Step("median %s %s, depth %d" % (form, S.name, depth), run, ref, leaves, S.name)


def _refined(S, row0=0, rows=None):
    """a stripe writes its own rows only: the others keep the fill"""
    r1 = S.ch if rows is None else row0 + rows

    def run(env, ctx):
        up = _devs(env, S)
        _layout_ok(env, S, up)
        c = env.full((S.ch, S.cws), FILL8, env.torch.uint8)
        ctx.MosaicImagesRefinedDev(up[1], up[2], up[3], up[4], S.h9s, c.data_ptr(), S.cw, S.ch, S.cws, row0, r1 - row0)
        return [c.cpu().numpy()]

    def ref(orc):
        full = S.rows_of(S.refined(orc))
        out = np.full_like(full, FILL8)
        out[row0:r1] = full[row0:r1]
        return [out]
    return Step("refined %s%s" % (S.name, "" if rows is None else ", rows %d .. %d" % (row0, r1 - 1)), run, ref, S.table(False, False, row0, rows), S.name)


def _feathered(S, cuts, ramp):
    def run(env, ctx):
        up = _devs(env, S)
        _layout_ok(env, S, up)
        c = env.full((S.ch, S.cws), FILL8, env.torch.uint8)
        for a, b in zip(cuts[:-1], cuts[1:]):
            ctx.MosaicFeatheredDev(up[1], up[2], up[3], up[4], S.h9s, c.data_ptr(), S.cw, S.ch, S.cws, a, b - a, ramp=ramp)
        return [c.cpu().numpy()]
    assert cuts[0] == 0 and cuts[-1] == S.ch
    return Step("feathered %s, %d stripe%s" % (S.name, len(cuts) - 1, "s" * (len(cuts) > 2)), run, lambda orc: [S.rows_of(S.feathered(orc, ramp))],
                S.table(True, False, cuts[-2], cuts[-1] - cuts[-2]), S.name)


def _median_cover(S, depth):
    def ref(orc):
        sel = S.median(orc, depth)[3]
        need = np.zeros(S.n, np.uint8)
        need[np.unique(sel[sel > 0]).astype(int) - 1] = 1
        return [need]
    return Step("median cover %s, depth %d" % (S.name, depth), lambda env, ctx: [np.asarray(ctx.MedianCover(S.w, S.h, S.h9s, depth=depth), np.uint8)], ref,
                S.table(True, False, used=True), S.name)


def _seamcut_cover(S):
    def run(env, ctx):
        d = env.once(("cells", S.name), lambda: env.dev(env.held[("cells_ref", S.name)]))
        return [np.asarray(ctx.SeamCutCover(S.w, S.h, S.h9s, d.data_ptr(), **S.p), np.uint8)]

    def ref(orc):
        own = S.seamcut(orc)["owner"]
        need = np.zeros(S.n, np.uint8)
        need[np.unique(own[own > 0]).astype(int) - 1] = 1
        return [need]
    return Step("seamcut cover %s" % S.name, run, ref, S.table(True, True, used=True), S.name)


# -- gains: tests/gain_ref.py, tests/block_gain_ref.py
def _tiles(S, step):
    """an upper bound that grows with the survey is all the plan needs of gain_tiles: the lattice points of the frames and of the pairs' frames"""
    return sum(-(-w // step) * -(-h // step) for w, h in zip(S.w, S.h)) + sum(-(-S.w[a] // step) * -(-S.h[a] // step) for a, b in S.pairs)


def _gain_stats(S, step):
    def run(env, ctx):
        up = _devs(env, S)
        st, cover = ctx.GainStatsDev(up[1], up[2], up[3], up[4], S.h9s, S.pairs, step)
        return [np.stack([st["a"], st["b"], st["n"]], 1).astype(np.int64), st["sum_a"].astype(np.int64), st["sum_b"].astype(np.int64), cover]

    def ref(orc):
        from tests import gain_ref as gr
        recs, cover = S._once(("gain", step), lambda: gr.stats_ref(S.maps(orc), S.pairs, step))
        return [np.array([[a, b, r[0]] for (a, b), r in zip(S.pairs, recs)], np.int64), np.array([r[1] for r in recs], np.int64), np.array([r[2] for r in recs], np.int64), cover]
    return Step("gain stats %s, step %d" % (S.name, step), run, ref, dict(gain_frames=S.n, gain_acc=7 * len(S.pairs) + S.n, gain_tiles=_tiles(S, step)), S.name)


def _block_geometry(S, orc):
    from tests import block_gain_ref as br
    sizes = list(zip(S.w, S.h))
    return sizes, S._once("coords", lambda: br.coord_maps(sizes, S.h9s)[0])


def _block_stats(S, step, gx, gy):
    fields = ("pair", "cell_a", "cell_b", "n")

    def run(env, ctx):
        up = _devs(env, S)
        st, cover = ctx.BlockGainStatsDev(up[1], up[2], up[3], up[4], S.h9s, S.pairs, step, gx, gy)
        return [np.stack([st[f] for f in fields], 1).astype(np.int64), st["sum_a"].astype(np.int64), st["sum_b"].astype(np.int64), st["reserved"].astype(np.int64), cover]

    def ref(orc):
        from tests import block_gain_ref as br
        sizes, coords = _block_geometry(S, orc)
        st, cover = S._once(("block", step, gx, gy), lambda: br.stats_ref(S.maps(orc), coords, sizes, S.pairs, step, gx, gy))
        return [np.stack([st[f] for f in fields], 1).astype(np.int64), st["sum_a"].astype(np.int64), st["sum_b"].astype(np.int64), np.zeros(len(st), np.int64), cover]
    cells = gx * gy
    return Step("block gain stats %s, step %d, grid %d x %d" % (S.name, step, gx, gy), run, ref,
                dict(gain_frames=S.n, gain_tiles=_tiles(S, step), block_gain_cover=S.n * cells, block_gain_acc=7 * len(S.pairs) * cells * cells), S.name)


def _gains_of(S, seed):
    g = np.random.default_rng(seed).uniform(0.7, 1.4, (S.n, 3)).astype(np.float32)
    g[0] = [0.0, 3.0, 1.0]                                                  # clamps at both ends
    return g


def _frames_back(ts, S, pad_fill=0xEE):
    out = []
    for t, w in zip(ts, S.w):
        a = t.cpu().numpy()
        assert np.all(a[:, 3 * w:] == pad_fill)                             # pitch padding untouched
        out.append(a[:, :3 * w].reshape(a.shape[0], w, 3))
    return out


def _apply_gains(S, seed, in_place):
    g = _gains_of(S, seed)

    def run(env, ctx):
        src = env.upload(S.imgs)
        dst = src if in_place else env.upload([np.full_like(a, 9) for a in S.imgs], fill=0xEE)
        ctx.ApplyGainsDev(src[1], dst[1], src[2], src[3], src[4], g)
        return _frames_back(dst[0], S)

    def ref(orc):
        from tests import gain_ref as gr
        return [gr.apply_lut(a, g[k]) for k, a in enumerate(S.imgs)]
    return Step("apply gains %s%s" % (S.name, ", in place" * in_place), run, ref, dict(gain_apply_frames=S.n), S.name)


def _apply_block_gains(S, seed, gx, gy):
    g = np.random.default_rng(seed).uniform(0.5, 1.7, (S.n, gy, gx, 3)).astype(np.float32)

    def run(env, ctx):
        src = env.upload(S.imgs)
        ctx.ApplyBlockGainsDev(src[1], src[1], src[2], src[3], src[4], g)
        return _frames_back(src[0], S)

    def ref(orc):
        from tests import block_gain_ref as br
        return [br.apply_ref(a, g[k]) for k, a in enumerate(S.imgs)]
    return Step("apply block gains %s, grid %d x %d" % (S.name, gx, gy), run, ref, dict(block_gain_apply_frames=S.n), S.name)


def _gain_compensate(S, step):
    """the gains are the host solve (float32 roundings of a float64 solution; tests/test_gpu_block_gain.py: within 2e-7 of gain_ref.solve_ref) of
    statistics that are the restatement's; the frames are the LUT of the gains returned, byte for byte"""
    def run(env, ctx):
        from tests import gain_ref as gr
        src = env.upload(S.imgs)
        g = ctx.GainCompensateDev(src[1], src[2], src[3], src[4], S.h9s, S.pairs, step=step)
        back = _frames_back(src[0], S)
        lut = [gr.apply_lut(a, g[k]) for k, a in enumerate(S.imgs)]
        return [g.view(np.uint32), np.array([np.array_equal(a, b) for a, b in zip(back, lut)])] + back

    def ref(orc):
        from tests import gain_ref as gr
        recs, cover = S._once(("gain", step), lambda: gr.stats_ref(S.maps(orc), S.pairs, step))
        st = np.zeros(len(S.pairs), np.dtype([("a", "<i4"), ("b", "<i4"), ("n", "<i8"), ("sum_a", "<i8", (3,)), ("sum_b", "<i8", (3,))]))
        for i, ((a, b), r) in enumerate(zip(S.pairs, recs)):
            st[i] = (a, b, r[0], r[1], r[2])
        assert np.isfinite(gr.solve_ref(st, cover)).all()                      # the system the gains solve has a solution
        return [None, np.ones(S.n, bool)] + [None] * S.n
    return Step("gain compensate %s, step %d" % (S.name, step), run, ref,
                dict(gain_frames=S.n, gain_acc=7 * len(S.pairs) + S.n, gain_tiles=_tiles(S, step), gain_apply_frames=S.n), S.name)


# -- overviews and previews: tests/overview_ref.py
def _overview(S, levels, nodata, host):
    """the levels of the seamline canvas under its count map; the host form stages canvas, map and levels in the ctx's overview buffers"""
    def run(env, ctx):
        from tests import overview_ref as ovr
        torch = env.torch
        canvas, count = env.held[("seamline_ref", S.name)]
        if host:
            lv, cv = ctx.MosaicOverview(canvas, S.cw, levels, valid=count, nodata=nodata, want_covers=True)
            return [a for pair in zip(lv, cv) for a in pair]
        dc, dm = env.once(("seamline_dev", S.name), lambda: (env.dev(canvas).view(S.ch, -1), env.dev(count)))
        geo = ovr.layout(S.cw, S.ch, levels)
        lv = [env.full((oh, ows), 0xA5, torch.uint8) for ow, oh, ows in geo]
        cv = [env.full((oh, ow), 0x2525, torch.int16) for ow, oh, ows in geo]
        ctx.MosaicOverviewDev(dc.data_ptr(), S.cw, S.ch, dc.shape[1], levels, [t.data_ptr() for t in lv], [t.data_ptr() for t in cv], d_valid_rows=dm.data_ptr(), nodata=nodata)
        ctx.synchronize()
        return [a for l, c in zip(lv, cv) for a in (l.cpu().numpy(), _u16(c))]

    def ref(orc):
        from tests import overview_ref as ovr
        out, _, count = S.seamline(orc)
        return [a for pair in ovr.overview_ref(S.rows_of(out, S.lws), S.cw, levels, nodata, count) for a in pair]
    leaves = dict(overview_canvas=S.ch * S.lws) if host else {}
    return Step("overview %s %s, %d levels, nodata %d" % ("host" if host else "device", S.name, levels, nodata), run, ref, leaves, S.name)


def _preview(S, render, level, nodata, stripe, ramp=0):
    """MosaicPreviewInto with "preview_stripe_rows" below the canvas's height: the render goes stripe by stripe through the frame table"""
    def run(env, ctx):
        from tests import overview_ref as ovr
        ow, oh, _ = ovr.layout(S.cw, S.ch, level)[-1]
        ctx.set_option("preview_stripe_rows", stripe)
        out = np.full((oh, 3 * ow + 29), TAIL, np.uint8)
        out, gw, gh, cover = ctx.MosaicPreviewInto(S.imgs, None, S.h9s, out=out, want_cover=True, render=render, ramp=ramp, level=level, nodata=nodata)
        ctx.set_option("preview_stripe_rows", 0)
        assert (gw, gh) == (ow, oh)
        return [out, cover]

    def ref(orc):
        from tests import overview_ref as ovr
        pix = (S.refined(orc), S.feathered(orc, ramp), S.seamline(orc, ramp)[0])[render]
        lv, cv = ovr.overview_ref(S.rows_of(pix, S.lws), S.cw, level, nodata, S.seamline(orc, ramp)[2])[level - 1]
        ow = cv.shape[1]
        out = np.full((lv.shape[0], 3 * ow + 29), TAIL, np.uint8)
        out[:, :3 * ow] = lv[:, :3 * ow]
        return [out, cv]
    assert stripe % (1 << level) == 0 and stripe < S.ch
    last = S.ch - (S.ch - 1) // stripe * stripe                             # the rows of the last stripe
    return Step("preview %s, render %d, level %d, nodata %d, stripes of %d" % (S.name, render, level, nodata, stripe), run, ref,
                dict(S.table(render > 0, render == 2, S.ch - last, last), preview_stripe=stripe * S.lws, into_srcs=S.src_bytes()), S.name)


def render_steps():
    """The order: large before small, the renders that upload different parts of the frame table (ramps, frame_of) next to each other, a
    seamline step directly before a seamcut step and the reverse (both write seamline_owner and follow frame_of), a refined step (no ramps,
    no frame_of) directly before a median and before a seamcut step on a survey with fewer frames than the ramps left behind."""
    V = render_surveys()
    L, W, S, B = V["L"], V["W"], V["S"], V["B"]
    return [
        _median(W, 9),                          # 130 table entries with ramps
        _seamcut(L, one_call=True),             # 12 entries, 4 list blocks, 43 x 39 cells in the ctx's own record and cell buffers
        _seamline(S),                           # 2 entries behind 12; 1 list block behind 4
        _seamcut(W, one_call=False),            # 6 x 6 cells behind 43 x 39; 130 entries
        _seamline_host(L),                      # the ctx's owner map: 337 x 310
        _seamcut_forms(S, "host"),              # ... 88 x 96 behind it; 22 x 24 cells
        _seamline_host(B),                      # ... 32 x 124 behind that
        _seamcut(L, one_call=False),            # the three entry points on the large survey
        _seamline(B, canvas=False),             # rows no frame touches
        _refined(L),                            # 12 entries, no ramps, no frame_of
        _median(S, 5),                          # 2 entries: behind them the refined frames of L, and ramps of an earlier render
        _refined(L, 100, 150),                  # a stripe: the frames that meet it
        _seamcut(S, one_call=True),             # 22 x 24 cells behind L's 43 x 39 in the ctx's own record and cell buffers
        _feathered(L, [0, 131, L.ch], 9),
        _feathered(B, [0, B.ch], 9),
        _seamline(B),
        _median_cover(W, 5),                    # 130 used flags
        _seamcut_cover(S),                      # 2
        _median_forms(L, "into", 5),            # into_srcs, into_canvas, the pinned download halves
        _seamcut_forms(S, "into"),
        _median_forms(L, "host", 5),            # mosaic_srcs, mosaic_canvas, the ctx's spread map
        _median_forms(B, "host", 2),
        _gain_stats(W, 1),                      # 130 frames, 100-odd pairs
        _gain_stats(S, 4),                      # 2 frames, 1 pair
        _block_stats(L, 2, 8, 6),               # 48 cells a frame
        _block_stats(S, 4, 2, 2),               # 4
        _apply_gains(L, 31, in_place=False),
        _apply_gains(S, 32, in_place=True),
        _apply_block_gains(L, 33, 8, 6),
        _apply_block_gains(S, 34, 1, 1),
        _gain_compensate(L, 2),
        _gain_compensate(S, 4),
        _overview(L, 5, 2, host=False),
        _overview(L, 5, 2, host=True),
        _overview(B, 7, 1, host=True),
        _preview(L, 2, 3, 2, 64),
        _preview(L, 1, 2, 0, 64, ramp=9),
        _preview(B, 0, 2, 1, 32),
    ]


def render_prepare(env, orc):
    """the host-side inputs some render steps take from the references: S's cell map, the seamline canvases and count maps of L and B"""
    V = render_surveys()
    env.held[("cells_ref", "S")] = V["S"].seamcut(orc)["cells"]
    for k in ("L", "B"):
        out, _, count = V[k].seamline(orc)
        env.held[("seamline_ref", k)] = (V[k].rows_of(out, V[k].lws), count)


# ==== the chip family: the multiband blend, plain and along optimised seams ==========================================================================
CHIP_SHARED = ("seamcut_labels", "seamcut_sums", "blend_seam_candidates", "blend_seam_cells", "chip_meta", "chip_imgs", "chip_masks", "chip_warp_args",
               "chip_warp_windows", "blend_canvas")
BAND = 5
_CHIP_CASES = {}


class ChipCase:
    """a case of tests/blend_seam_patterns.py with its numbers: chips, the blend's grid and canvas, the chips' bytes"""

    def __init__(self, name):
        from tests import blend_seam_patterns as bp
        self.name, self.case = name, bp.CASES[name]()
        self.imgs, self.h9s, self.p, self.keep = [np.ascontiguousarray(a) for a in self.case.imgs], np.asarray(self.case.h9s, np.float32), self.case.p, self.case.keep
        self._own = None

    def ref(self, orc):
        """(cells given by the case or None, the restatement's dict), tests/blend_seam_patterns.reference's cache"""
        from tests import blend_seam_patterns as bp
        _, cells, r = bp.reference(orc, self.name)
        return cells, r

    def own(self, orc):
        """the restatement under the label stage's own map (the case's, where it gives no map)"""
        from tests import blend_seam_ref as bs
        cells, r = self.ref(orc)
        if cells is None:
            return r
        if self._own is None:
            self._own = bs.blend_seam_ref(orc, self.imgs, self.h9s, self.p, keep=self.keep, cells=None, chips=r["set"])
        return self._own

    # the case's own numbers, from the frames' sizes and transforms alone (translations: a chip is its frame's box)
    def numbers(self):
        live = [k for k in range(len(self.imgs)) if (self.keep is None or self.keep[k]) and self.h9s[k, 8] != 0]
        t = self.h9s.reshape(-1, 3, 3)
        assert all(np.array_equal(t[k, :2, :2], np.eye(2, dtype=np.float32)) for k in live)
        x0 = min(float(t[k, 0, 2]) for k in live); y0 = min(float(t[k, 1, 2]) for k in live)
        cw = int(np.ceil(max(float(t[k, 0, 2]) + self.imgs[k].shape[1] for k in live) - x0))
        ch = int(np.ceil(max(float(t[k, 1, 2]) + self.imgs[k].shape[0] for k in live) - y0))
        s = 1 << self.p["level"]
        return dict(chips=len(live), cw=cw, ch=ch, cells=-(-cw // s) * -(-ch // s), chip_bytes=sum(self.imgs[k].shape[0] * ((3 * self.imgs[k].shape[1] + 3) & ~3) for k in live),
                    mask_bytes=sum(self.imgs[k].shape[0] * ((self.imgs[k].shape[1] + 3) & ~3) for k in live), canvas=ch * ((3 * cw + 3) & ~3))


def chip_cases():
    """M many130 (130 chips of 16 x 16: several batches), G big (twelve 128 x 96 frames, canvas 337 x 310), C crafted3, K keep_drops (a caller's
    map, a dropped frame), T thin_named1 (a caller's map; chips whose distance map is 0 / 0)"""
    if not _CHIP_CASES:
        for key, name in (("M", "many130"), ("G", "big"), ("C", "crafted3"), ("K", "keep_drops"), ("T", "thin_named1")):
            _CHIP_CASES[key] = ChipCase(name)
    return _CHIP_CASES


def _mosaic_survey(X):
    """the same frames as a survey of the seamline family: SeamCellsDev works on the mosaic canvas's grid"""
    return _SURVEYS.setdefault("chip " + X.name, Survey("chip " + X.name, X.imgs, X.h9s, X.p, []))


def _chip_frames(env, X):
    return env.once(("chip frames", X.name), lambda: env.upload(X.imgs))


def _set_arrays(r):
    """a chip set as arrays: the rectangles and images of the chips, the canvas, every chip and every mask"""
    info = np.array([[int(c[k]) for k in ("x0", "y0", "w", "h", "img")] for c in r["chips"]], np.int64).reshape(-1, 5)
    return [info, np.array([r["cw"], r["ch"]], np.int64)] + [np.asarray(a) for a in r["chip_imgs"]] + [np.asarray(a) for a in r["masks"]]


def _table_of(X, nums):
    return dict(chip_meta=nums["chips"], chip_imgs=nums["chip_bytes"], chip_masks=nums["mask_bytes"], chip_warp_args=nums["chips"])


def _seam_cells_mosaic(X, tag):
    """SeamCellsDev on the mosaic canvas's grid: mi_seam_labels_dev's buffers, as BlendSeamCellsDev's"""
    S = _mosaic_survey(X)
    gw, gh = S.grid()

    def run(env, ctx):
        up = _chip_frames(env, X)
        assert env.im.seam_grid(up[2], up[3], S.h9s, S.p["level"]) == (gw, gh)
        t = env.full((gw * gh,), 0x1111, env.torch.int16)
        rep = ctx.SeamCellsDev(up[1], up[2], up[3], up[4], S.h9s, t.data_ptr(), gw, gh, **S.p)
        return [_u16(t).reshape(gh, gw), rep]

    def ref(orc):
        r = S.seamcut(orc)
        return [r["cells"], r["report"]]
    return Step("mosaic cells %s, %s" % (X.name, tag), run, ref, dict(S.table(True, True), seamcut_labels=gw * gh, seamcut_sums=8 * gw * gh), X.name)


def _blend_cells(X):
    nums = X.numbers()

    def run(env, ctx):
        torch = env.torch
        up = _chip_frames(env, X)
        gw, gh = env.im.blend_seam_grid(up[2], up[3], X.h9s, X.p["level"], X.keep)
        assert gw * gh == nums["cells"]
        d_cand = env.full((gh * gw * 32,), 0xAB, torch.uint8)
        d_cells = env.full((gh * gw,), 0x7777, torch.int16)
        rep = ctx.BlendSeamCellsDev(up[1], up[2], up[3], up[4], X.h9s, d_cells.data_ptr(), gw, gh, keep=X.keep, d_cand=d_cand.data_ptr(), **X.p)
        return [d_cand.cpu().numpy().reshape(gh, gw, 32), _u16(d_cells).reshape(gh, gw), rep]

    def ref(orc):
        r = X.ref(orc)[1]
        return [r["records"], r["cells"], r["report"]]
    return Step("blend cells %s" % X.name, run, ref, dict(_table_of(X, nums), seamcut_labels=nums["cells"], seamcut_sums=8 * nums["cells"]), X.name)


def _chips_seam(X, given, hold=None):
    """ChipsAndMasksSeam under the case's map (given) or under the one made inside the call"""
    nums = X.numbers()

    def run(env, ctx):
        cells = env.held[("given", X.name)] if given else None
        r = ctx.ChipsAndMasksSeam(X.imgs, X.h9s, keep=X.keep, cells=cells, **X.p)
        if hold:
            env.held.setdefault(hold, r)
        return _set_arrays(r)

    def ref(orc):
        r = X.ref(orc)[1] if given else X.own(orc)
        return _set_arrays(dict(r["set"], masks=r["masks"]))
    leaves = dict(_table_of(X, nums), blend_seam_cells=nums["cells"])
    if not given:
        leaves.update(blend_seam_candidates=nums["cells"], seamcut_labels=nums["cells"], seamcut_sums=8 * nums["cells"])
    return Step("chips and masks along seams %s, %s map" % (X.name, "the caller's" if given else "its own"), run, ref, leaves, X.name)


def _blend_held(X, hold, given):
    """MultiBandBlend of the chips an earlier step holds"""
    nums = X.numbers()

    def run(env, ctx):
        r = env.held[hold]
        got, ow, oh, ows = ctx.MultiBandBlend(r["chips"], r["chip_imgs"], r["masks"], r["cw"], r["ch"], band=BAND)
        return [got, np.array([ow, oh, ows], np.int64)]

    def ref(orc):
        c = (X.ref(orc)[1] if given else X.own(orc))["canvas"]
        return [c, np.array([nums["cw"], nums["ch"], c.shape[1]], np.int64)]
    return Step("blend of the held chips of %s" % X.name, run, ref, dict(blend_canvas=nums["canvas"], chip_imgs=nums["chip_bytes"], chip_masks=nums["mask_bytes"]), X.name)


def _blended_seam(X, form, given=False, tag=""):
    """the one-call forms: device (the case's map where `given`, else made inside), host, _into (a wider row whose tail stays)"""
    nums = X.numbers()

    def run(env, ctx):
        im, torch = env.im, env.torch
        if form == "host":
            r = ctx.MosaicBlendedSeam(X.imgs, X.h9s, keep=X.keep, band=BAND, **X.p)
            return [r[0], np.array(r[1:], np.int64)]
        w, h = [a.shape[1] for a in X.imgs], [a.shape[0] for a in X.imgs]
        cw, ch, cws = im.blend_layout(w, h, X.h9s, X.keep)
        assert (cw, ch, ch * cws) == (nums["cw"], nums["ch"], nums["canvas"])
        if form == "into":
            out = np.full((ch, cws + 8), TAIL, np.uint8)
            ctx.MosaicBlendedSeamInto(X.imgs, None, X.h9s, keep=X.keep, band=BAND, out=out, pitch=cws + 8, **X.p)
            return [out]
        up = _chip_frames(env, X)
        d_map = env.once(("given dev", X.name), lambda: env.dev(env.held[("given", X.name)])) if given else None
        t = env.full((ch, cws), FILL8, torch.uint8)
        ctx.MosaicBlendedSeamDev(up[1], up[2], up[3], up[4], X.h9s, t.data_ptr(), cw, ch, cws, keep=X.keep, band=BAND, d_cells=d_map.data_ptr() if given else 0, **X.p)
        return [t.cpu().numpy()]

    def ref(orc):
        c = (X.ref(orc)[1] if given else X.own(orc))["canvas"]
        if form == "host":
            return [c, np.array([nums["cw"], nums["ch"], c.shape[1]], np.int64)]
        if form == "into":
            out = np.full((c.shape[0], c.shape[1] + 8), TAIL, np.uint8)
            out[:, :3 * nums["cw"]] = c[:, :3 * nums["cw"]]
            return [out]
        return [c]
    leaves = dict(_table_of(X, nums), blend_canvas=nums["canvas"], blend_seam_cells=nums["cells"])
    if form == "device":
        leaves.update(chip_warp_windows=nums["chips"])                     # the deferred chips' windows: at most one entry a chip
    if not given:
        leaves.update(blend_seam_candidates=nums["cells"], seamcut_labels=nums["cells"], seamcut_sums=8 * nums["cells"])
    return Step("blended along seams %s, %s%s" % (X.name, form, tag), run, ref, leaves, X.name)


class PlainCase:
    """a chips survey of tests/warp_patterns.py or tests/blend_edges.py for the plain forms, against the oracle"""

    def __init__(self, name, case):
        self.name, self.case = name, case
        self.imgs, self.h9s, self.keep = [np.ascontiguousarray(a) for a in case.imgs], np.asarray(case.h9s, np.float32), case.keep
        self._c = {}

    def chips(self, orc):
        if "chips" not in self._c:
            self._c["chips"] = orc.chips_and_masks(self.imgs, self.h9s, keep=self.keep, find_masks=True)
        return self._c["chips"]

    def canvas(self, orc, band):
        if band not in self._c:
            o = self.chips(orc)
            self._c[band] = (orc.multiband_blend(o["chips"], o["chip_imgs"], o["masks"], o["cw"], o["ch"], band=band)[0], o["cw"], o["ch"])
        return self._c[band]


def plain_cases():
    if "seventy" not in _CHIP_CASES:
        from tests import blend_edges as be
        from tests import warp_patterns as wp
        _CHIP_CASES["seventy"] = PlainCase("seventy", next(c for c in wp.chips_cases() if c.tag == "seventy"))
        _CHIP_CASES["strip"] = PlainCase("strip", next(s for s in be.survey_cases() if s.tag == "strip"))
    return _CHIP_CASES["seventy"], _CHIP_CASES["strip"]


def _plain_chips(P):
    def run(env, ctx):
        return _set_arrays(ctx.ChipsAndMasks(P.imgs, P.h9s, keep=P.keep, find_masks=True))
    n = len(P.imgs)
    return Step("plain chips and masks %s" % P.name, run, lambda orc: _set_arrays(P.chips(orc)),
                dict(chip_meta=n, chip_warp_args=n, chip_imgs=sum(a.shape[0] * ((3 * a.shape[1] + 3) & ~3) for a in P.imgs),
                     chip_masks=sum(a.shape[0] * ((a.shape[1] + 3) & ~3) for a in P.imgs)), P.name)


def _plain_blended(P, row0=0):
    """MosaicBlendedDev, the whole canvas or (row0 > 0) the stripe from row0 to its end, against the oracle's blend (the columns of the
    canvas; the library returns its rows)"""
    def run(env, ctx):
        up = env.once(("plain frames", P.name), lambda: env.upload(P.imgs, pad=0))
        ch = env.im.blend_layout(up[2], up[3], P.h9s, P.keep)[1]
        assert 32 < row0 < 64 <= ch or row0 == 0
        got, cw, ch, cws = ctx.MosaicBlendedDev(up[1], up[2], up[3], up[4], P.h9s, keep=P.keep, band=BAND, **(dict(row0=row0, rows=ch - row0) if row0 else {}))
        return [got.cpu().numpy()[:, :3 * cw], np.array([cw, ch], np.int64)]

    def ref(orc):
        c, cw, ch = P.canvas(orc, BAND)
        return [c[row0:, :3 * cw], np.array([cw, ch], np.int64)]
    n = len(P.imgs)
    return Step("plain blended %s%s" % (P.name, ", from row %d" % row0 if row0 else ""), run, ref, dict(chip_meta=n, chip_warp_args=n, chip_warp_windows=n), P.name)


def chip_steps():
    """The large case first, then the smallest, then the large one again; SeamCellsDev of the same survey on the mosaic grid directly before and
    directly after BlendSeamCellsDev (both go through mi_seam_labels_dev's buffers); the plain forms between the seam forms."""
    X = chip_cases()
    M, G, C, K, T = X["M"], X["G"], X["C"], X["K"], X["T"]
    seventy, strip = plain_cases()
    return [
        _blended_seam(G, "device", tag=", first"),         # 12 chips of 128 x 96, canvas 337 x 310, 22 x 20 cells
        _blended_seam(T, "device", given=True),            # 4 chips, three of them with a 0 / 0 distance map; canvas 64 x 48
        _seam_cells_mosaic(C, "before"),                   # 22 x 34 cells on the mosaic grid
        _blend_cells(C),                                   # ... and on the blend's
        _seam_cells_mosaic(C, "after"),
        _seam_cells_mosaic(M, "before"),                   # 6 x 6 cells behind 22 x 34; 130 frames
        _blend_cells(M),
        _seam_cells_mosaic(M, "after"),
        _chips_seam(M, given=False),                       # 130 chips: several batches
        _chips_seam(K, given=True, hold="held K"),         # 2 chips behind 130; a map that names the dropped frame everywhere
        _blend_held(K, "held K", given=True),
        _blended_seam(C, "host"),
        _plain_chips(seventy),                             # 70 chips, three batches of candidates
        _blended_seam(K, "into"),                          # the map made inside the call
        _plain_blended(strip),
        _plain_blended(strip, 49),                         # a stripe cut inside the second 2^5 block of rows
        _blend_cells(G),
        _blend_cells(T),
        _chips_seam(C, given=False, hold="held C"),
        _plain_chips(plain_thin()),
        _blend_held(C, "held C", given=False),
        _blended_seam(M, "device"),
        _blended_seam(T, "host"),
        _blended_seam(G, "device", tag=", again"),         # equals its first run
    ]


def plain_thin():
    if "thin" not in _CHIP_CASES:
        from tests import warp_patterns as wp
        _CHIP_CASES["thin"] = PlainCase("thin", next(c for c in wp.chips_cases() if c.tag == "thin"))
    return _CHIP_CASES["thin"]


def chip_prepare(env, orc):
    """the caller's cell maps of the cases that give one"""
    for X in chip_cases().values():
        if isinstance(X, ChipCase) and X.ref(orc)[0] is not None:
            env.held[("given", X.name)] = X.ref(orc)[0]


# ==== the record family: tie refinement, local registration, undistortion, verification, guided matching, the screen, the two LM loops ==============
PAIR_SHARED = ("tie_records", "tie_ties", "tie_outputs", "local_warp_frames", "local_warp_nodes", "local_warp_records", "undistort_frames", "verify_edges",
               "verify_cycles", "verify_residuals", "verify_records", "guided_pairs", "guided_keypoints", "pair_results", "screen_frames", "ag_res_compact",
               "proj_compact", "calib_compact", "proj_blocks", "calib_blocks", "moments_records")
DIST, SEED = 2.5, 12345
# (ag_res_counts has one size for every call; what differs between the calls that share it is the length of <prefix>_compact and _blocks:
# proj_compact, calib_compact, proj_blocks and calib_blocks below)
_PAIR = {}


def _raw(a):
    return np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8)


def _pair_once(key, make):
    if key not in _PAIR:
        _PAIR[key] = make()
    return _PAIR[key]


def _env3(env, ctx):
    """the (torch, im, ctx) triple the helpers of tests/test_gpu_local_warp.py and tests/test_gpu_undistort.py take"""
    return env.torch, env.im, ctx


def _recs_dev(env, recs):
    t = env.torch.from_numpy(np.ascontiguousarray(recs).view(np.uint8).reshape(len(recs), -1).copy()).cuda()
    env.torch.cuda.synchronize()
    return t


def _guarded(env, n, itemsize):
    """n records of device output and one record of guard behind them"""
    return env.full((n + 1, itemsize), 0xCD, env.torch.uint8)


def _unguard(t, n):
    a = t.cpu().numpy()
    assert (a[n:] == 0xCD).all(), "the guard record behind the output was written"
    return a[:n]


# -- tie refinement: tests/tie_refine_ref.py
def tie_cases():
    """frames of 96 x 80; `six`: six records of 1, 63, 64, 65, 399 and 400 ties; `three`: three records of a few ties; `one`: one record of one tie"""
    def make():
        from tests import tie_refine_cases as tc
        from tests.test_gpu_tie_refine import ROT, pair_case
        imgs, big = pair_case(96, 80, 96, 80, ROT, 400, 4, margin=9.0)

        def cut(n_in, first=0):
            r = big.copy()
            r["a"][:n_in], r["b"][:n_in] = big["a"][first:first + n_in], big["b"][first:first + n_in]
            r["n_in"] = n_in
            r["a"][n_in:] = 0
            r["b"][n_in:] = 0
            return r
        return dict(imgs=imgs, six=tc.records(*[cut(n) for n in (1, 63, 64, 65, 399, 400)]), three=tc.records(cut(5, 40), cut(9, 80), cut(2, 120)), one=tc.records(cut(1, 200)))
    return _pair_once("tie", make)


def _refine_ties(which, form, radius, search):
    """form: "device" (out of place), "in place", "host" (RefineTies: host records and host images through tie_records, tie_outputs, tie_srcs)"""
    T = tie_cases()
    recs = T[which]
    p = dict(radius=radius, search=search)

    def run(env, ctx):
        from tests.test_gpu_tie_refine import DevFrames, run_dev
        if form == "host":
            return [_raw(v) for v in ctx.RefineTies(recs.copy(), T["imgs"], **p)]
        fr = env.once("tie frames", lambda: DevFrames(env.torch, T["imgs"]))
        out = [_raw(v) for v in run_dev(ctx, env.torch, recs, fr, inplace=form == "in place", **p)]
        assert fr.unchanged()
        return out

    def ref(orc):
        from tests import tie_refine_ref as tr
        return [_raw(v) for v in _pair_once(("tie ref", which, radius, search), lambda: tr.refine_ties(recs, T["imgs"], **p))]
    n, ties = len(recs), int(recs["n_in"].max())
    return Step("refine ties %s, %s" % (which, form), run, ref, dict(tie_records=n, tie_outputs=n, tie_ties=ties), "tie " + which)


# -- local registration and undistortion: tests/local_warp_ref.py, tests/undistort_ref.py
def warp_surveys():
    from tests import local_warp_cases as lc
    return _pair_once("warp", lambda: dict(six=lc.survey(seed=2), two=lc.survey(seed=1, n=2)))


def _frames_of(s, seed):
    return [np.random.default_rng(seed + k).integers(0, 256, (s["h"][k], s["w"][k], 3), dtype=np.uint8) for k in range(s["n"])]


def _residual_stats(which, gx, gy):
    s = warp_surveys()[which]
    p = dict(grid_x=gx, grid_y=gy)

    def run(env, ctx):
        from tests.test_gpu_local_warp import stats_dev
        return [stats_dev(_env3(env, ctx), s["rec"], s["w"], s["h"], s["h9s"], **p)]

    def ref(orc):
        from tests import local_warp_ref as lr
        return [_pair_once(("lw stats", which, gx, gy), lambda: lr.stats(s["rec"], s["w"], s["h"], s["h9s"], **p))]
    return Step("residual stats %s, grid %d x %d" % (which, gx, gy), run, ref,
                dict(local_warp_frames=s["n"], local_warp_nodes=s["n"] * (gx + 1) * (gy + 1), local_warp_records=len(s["rec"])), "warp " + which)


def _local_register(which, gx, gy):
    """the grids to their Q8 nodes (the solve is float64 on the host; the nodes are what the apply reads), the frames byte for byte"""
    s = warp_surveys()[which]
    p = dict(grid_x=gx, grid_y=gy)
    imgs = _frames_of(s, 300)

    def run(env, ctx):
        from tests import local_warp_ref as lr
        from tests.test_gpu_local_warp import frames_to_device
        dev = frames_to_device(env.torch, imgs)
        d_rec = _recs_dev(env, s["rec"])
        g, rep = ctx.LocalRegisterDev(d_rec.data_ptr(), len(s["rec"]), [t.data_ptr() for t in dev], s["w"], s["h"], [3 * x + 4 for x in s["w"]], s["h9s"], **p)
        out = [lr.node_q8(g), np.asarray(rep["n_ties"], np.int64), np.asarray(rep["solved"], np.int64)]
        for k, t in enumerate(dev):
            full = t.cpu().numpy()
            assert (full[:, 3 * s["w"][k]:] == 66).all()
            out.append(full[:, :3 * s["w"][k]].reshape(imgs[k].shape))
        return out

    def ref(orc):
        from tests import local_warp_ref as lr

        def make():
            st = lr.stats(s["rec"], s["w"], s["h"], s["h9s"], **p)
            grids, _, reps = lr.solve(st, s["n"], **dict(lr.DEFAULTS, **p))
            return [lr.node_q8(grids), np.array([r["n_ties"] for r in reps], np.int64), np.array([r["solved"] for r in reps], np.int64)] + \
                   [lr.apply(imgs[k], grids[k])[0] for k in range(s["n"])]
        return _pair_once(("lw register", which, gx, gy), make)
    return Step("local register %s, grid %d x %d" % (which, gx, gy), run, ref,
                dict(local_warp_frames=s["n"], local_warp_nodes=s["n"] * (gx + 1) * (gy + 1), local_warp_records=len(s["rec"])), "warp " + which)


def _apply_warps(tag, sizes, gx, gy, in_place):
    imgs = [np.random.default_rng(500 + k).integers(0, 256, (h, w, 3), dtype=np.uint8) for k, (w, h) in enumerate(sizes)]
    grids = [np.random.default_rng(600 + k).uniform(-3.0, 3.0, (gy + 1, gx + 1, 2)).astype(np.float32) for k in range(len(sizes))]

    def run(env, ctx):
        from tests.test_gpu_local_warp import run_apply
        got, cnt = run_apply(_env3(env, ctx), imgs, grids, in_place)
        return [np.asarray(cnt, np.int64)] + got

    def ref(orc):
        from tests import local_warp_ref as lr
        want = _pair_once(("lw apply", tag), lambda: [lr.apply(i, g) for i, g in zip(imgs, grids)])
        return [np.array([n for _, n in want], np.int64)] + [a for a, _ in want]
    return Step("apply local warps %s" % tag, run, ref, dict(local_warp_frames=len(sizes), local_warp_nodes=len(sizes) * (gx + 1) * (gy + 1)), "apply " + tag)


def _undistort(tag, w, h, n, in_place):
    imgs = [np.random.default_rng(700 + k).integers(0, 256, (h, w, 3), dtype=np.uint8) for k in range(n)]

    def cam():
        from tests import undistort_ref as ur
        return ur.cameras_for(w, h)["pincushion"]

    def run(env, ctx):
        from tests.test_gpu_undistort import run_dev
        got, cnt = run_dev(_env3(env, ctx), imgs, cam(), in_place=in_place)
        return [np.asarray(cnt, np.int64)] + got

    def ref(orc):
        from tests import undistort_ref as ur
        want = _pair_once(("undistort", tag), lambda: [ur.undistort(i, cam()) for i in imgs])
        return [np.array([c for _, c in want], np.int64)] + [a for a, _ in want]
    return Step("undistort %s" % tag, run, ref, dict(undistort_frames=n), "undistort " + tag)


# -- pair verification: tests/verify_ref.py
def _pair_edges(count):
    def run(env, ctx):
        from tests import verify_cases as vc
        im = env.im
        d_r = env.once("verify edge records", lambda: _recs_dev(env, vc.edge_records()))
        d_e = _guarded(env, count, im.PAIR_EDGE.itemsize)
        ctx.PairEdgesDev(d_r.data_ptr(), count, vc.EDGE_IMAGES, d_e.data_ptr())
        ctx.synchronize()
        return [_unguard(d_e, count)]

    def ref(orc):
        from tests import verify_cases as vc
        from tests import verify_ref as vr
        want = _pair_once("verify edges", lambda: vr.edges(vc.edge_records(), vc.EDGE_IMAGES))
        return [_raw(want[:count]).reshape(count, -1)]
    return Step("pair edges, %d records" % count, run, ref, dict(verify_records=count), "edges %d" % count)


def _pair_residuals(count):
    def run(env, ctx):
        from tests import verify_cases as vc
        im = env.im
        h9, label = vc.edge_transforms()
        d_r = env.once("verify edge records", lambda: _recs_dev(env, vc.edge_records()))
        d_o = _guarded(env, count, im.PAIR_RESIDUAL.itemsize)
        ctx.PairResidualsDev(d_r.data_ptr(), count, h9, label, d_o.data_ptr())
        ctx.synchronize()
        return [_unguard(d_o, count)]

    def ref(orc):
        from tests import verify_cases as vc
        from tests import verify_ref as vr
        want = _pair_once("verify residuals", lambda: vr.residuals(vc.edge_records(), *vc.edge_transforms()))
        return [_raw(want[:count]).reshape(count, -1)]
    return Step("pair residuals, %d records" % count, run, ref, dict(verify_residuals=count, verify_records=count), "residuals %d" % count)


def _pair_cycles(tag, make):
    def graph():
        return _pair_once(("graph", tag), make)

    def ref(orc):
        from tests import verify_ref as vr
        edg, n = graph()
        return [_raw(_pair_once(("cycles", tag), lambda: vr.cycles(edg, n, 6.0)))]
    return Step("pair cycles, %s" % tag, lambda env, ctx: [_raw(ctx.PairCyclesDev(graph()[0], graph()[1], 6.0))], ref,
                dict(verify_edges=len(graph()[0]), verify_cycles=len(graph()[0])), "cycles " + tag)


def _verify_pairs(name, seed, pct):
    """the decisions against tests/verify_ref.py; the records and transforms, which come out of the host alignment, against the host twin"""
    def survey():
        from tests import verify_cases as vc
        return _pair_once(("verify survey", name, seed, pct), lambda: vc.survey(name, seed, pct))

    def run(env, ctx):
        im = env.im
        s = survey()
        recs = s["recs"]
        d_r = _recs_dev(env, recs)
        d_o = _guarded(env, len(recs), im.PAIR_RESULT.itemsize)
        label, tr, rep, summ = ctx.VerifyPairsDev(d_r.data_ptr(), len(recs), s["n"], d_o.data_ptr())
        return [np.asarray(rep["verdict"], np.int64), np.asarray(label, np.int64), np.asarray(rep["round"], np.int64), np.asarray(rep["n_ok"], np.int64),
                np.asarray(rep["n_bad"], np.int64), _raw(rep["min_e2"]), np.array([int(summ["rounds"])]), _unguard(d_o, len(recs)), _raw(tr)]

    def ref(orc):
        import imagemosaicing_amd as im
        from tests import verify_ref as vr
        s = survey()
        r = _pair_once(("verify ref", name, seed, pct), lambda: vr.verify(s["recs"], s["n"]))
        h_out, _, h_tr, _, _ = _pair_once(("verify host", name, seed, pct), lambda: im.verify_pairs_results(s["recs"], s["n"]))
        return [np.asarray(r["verdict"], np.int64), np.asarray(r["label"], np.int64), np.asarray(r["round"], np.int64), np.asarray(r["n_ok"], np.int64),
                np.asarray(r["n_bad"], np.int64), _raw(r["min_e2"]), np.array([int(r["rounds"])]), _raw(h_out).reshape(len(h_out), -1), _raw(h_tr)]
    n = len(survey()["recs"])
    return Step("verify pairs %s, %d %% wrong" % (name, pct), run, ref, dict(verify_records=n, verify_edges=n, verify_cycles=n, verify_residuals=n), "verify " + name)


# -- guided matching and the plain pair stage on the same features: tests/guided_ref.py, tests/match_patterns.py
def guided_scenes(which):
    from tests import guided_cases as gc
    if which == "six":
        return _pair_once("guided six", lambda: [gc.scene(500 + k, 80 + 9 * k, 120 - 5 * k, G) for k, G in
                                                 enumerate((gc.SHIFT, gc.IDENTITY, gc.PROJECTIVE, gc.SIMILARITY, gc.SHIFT, gc.ZERO_DEN))])
    return _pair_once("guided tiny", lambda: [gc.scene(77, 3, 3, gc.SHIFT, true=1.0, wrong=0.0)])


def _guided(which, n_pairs):
    """GuidedSelectDev and GuidedMatchDev over n_pairs pairs (the scenes in turn, the same pair several times among them): lists, counts,
    distances, and the records without their _pad word as in tests/test_gpu_guided.py"""
    def order():
        scenes = guided_scenes(which)
        return [(5 * p + p // 7) % len(scenes) for p in range(n_pairs)]

    def run(env, ctx):
        from tests import guided_ref as gr
        from tests.test_gpu_guided import _install_case, _match_dev, _select_dev
        scenes = guided_scenes(which)
        ids = [_install_case(ctx, k, s) for k, s in enumerate(scenes)]
        pairs, guides = [ids[k] for k in order()], [scenes[k]["G"] for k in order()]
        a, b, ns, dd = _select_dev(ctx, pairs, guides)
        recs = _match_dev(ctx, pairs, guides)
        ctx.DropFeatures(-1)
        return [_raw(a), _raw(b), ns.astype(np.int64), _raw(dd), np.stack([np.frombuffer(gr.record_bytes(r), np.uint8) for r in recs])]

    def ref(orc):
        from tests import guided_cases as gc
        from tests import guided_ref as gr
        from tests import oracle_lib as ol
        scenes = guided_scenes(which)

        def make():
            fast = ol.load_oracle_fast()
            sel = [gr.lists_400(*gc.ref_select(s)) for s in scenes]
            nsel = [len(gc.ref_select(s)[0]) for s in scenes]
            rec = [gr.record(fast, 2 * k, 2 * k + 1, s["xy_i"], s["d_i"], s["xy_j"], s["d_j"], s["G"], DIST, SEED, **dict(gr.DEFAULTS, **s["params"])) for k, s in enumerate(scenes)]
            return sel, nsel, rec
        sel, nsel, rec = _pair_once(("guided ref", which), make)
        o = order()
        return [_raw(np.stack([sel[k][0] for k in o])), _raw(np.stack([sel[k][1] for k in o])), np.array([nsel[k] for k in o], np.int64),
                _raw(np.stack([sel[k][2] for k in o])), np.stack([np.frombuffer(gr.record_bytes(rec[k]), np.uint8) for k in o])]
    kps = max(max(len(s["xy_i"]), len(s["xy_j"])) for s in guided_scenes(which))
    return Step("guided select and match %s, %d pairs" % (which, n_pairs), run, ref, dict(guided_pairs=n_pairs, pair_results=n_pairs, guided_keypoints=kps), "guided " + which)


def _match_plain(which):
    """MatchPairsDev on the features of the guided scenes: mi_ransac_batch and mi_finalize_pairs, which the guided stage goes through as well"""
    def run(env, ctx):
        from tests.test_gpu_guided import _install_case
        im = env.im
        scenes = guided_scenes(which)
        ids = [_install_case(ctx, k, s) for k, s in enumerate(scenes)]
        d_o = _guarded(env, len(ids), im.PAIR_RESULT.itemsize)
        ctx.MatchPairsDev(ids, d_o.data_ptr(), DIST, SEED)
        ctx.synchronize()
        ctx.DropFeatures(-1)
        out = []
        for r in _unguard(d_o, len(ids)).reshape(-1).view(im.PAIR_RESULT):
            n = int(r["n_in"])
            assert not _raw(r["a"][n:]).any() and not _raw(r["b"][n:]).any()
            out += [np.array([r["i"], r["j"], r["n_selected"], n, r["accepted"], r["ok"]], np.int64), _raw(r["a"][:n]), _raw(r["b"][:n]), _raw(r["H"])]
        return out

    def ref(orc):
        from tests import guided_cases as gc
        from tests import match_patterns as mp
        from tests import oracle_lib as ol

        def make():
            fast = ol.load_oracle_fast()
            out = []
            for k, s in enumerate(guided_scenes(which)):
                o = mp.oracle_pair_record(fast, s["xy_i"], s["d_i"], s["xy_j"], s["d_j"], gc.W, gc.H, DIST, SEED)
                H = o["H"] if o["accepted"] else np.zeros(9, np.float32)         # a rejected record: H all zero, ok 0 (include/mi355_mosaic.h)
                out += [np.array([2 * k, 2 * k + 1, o["n_selected"], o["n_in"], o["accepted"], o["ok"] if o["accepted"] else 0], np.int64), _raw(o["a"]), _raw(o["b"]),
                        _raw(np.asarray(H, np.float32))]
            return out
        return _pair_once(("match ref", which), make)
    n = len(guided_scenes(which))
    return Step("plain match pairs %s" % which, run, ref, dict(pair_results=n), "match " + which)


# -- the descriptor screen: tests/screen_ref.py
def _screen(count, top_k=96, ratio=80):
    def frames():
        from tests import screen_patterns as sp
        return _pair_once("screen frames", sp.nn_frames)

    def run(env, ctx):
        from tests import screen_patterns as sp
        ids = np.arange(count, dtype=np.int32) * 3 + 5
        for i, f in zip(ids, frames()[:count]):
            ctx.SetFeatures(int(i), f["kp"], f["desc"].astype(np.float32), sp.W, sp.H)
        buf = env.full((count * count + count,), 0x5A5A5A5A, env.torch.int32)
        ctx.ScreenScoresDev(ids, buf.data_ptr(), window=0, top_k=top_k, ratio_pct=ratio)
        ctx.synchronize()
        ctx.DropFeatures(-1)
        h = buf.cpu().numpy()
        assert (h[count * count:] == 0x5A5A5A5A).all()
        return [h[:count * count].reshape(count, count)]

    def ref(orc):
        from tests import screen_patterns as sp
        from tests import screen_ref as sr
        return [_pair_once(("screen ref", count), lambda: sr.score_matrix([sp.ref_list(f, top_k) for f in frames()[:count]], ratio, 0))]
    assert 2 <= count <= len(frames())
    return Step("screen scores, %d frames" % count, run, ref, dict(screen_frames=count), "screen %d" % count)


# -- compaction, moments, the block entry points and the two LM loops: the host twins, bit for bit
def lm_records(which):
    """edge: the 257 records of tests/projective_cases.edge_records with parameters for 48 images; calib_edge: those of tests/calib_cases.py;
    grid16 / strip12: a survey of each case module with three records that are not accepted among them"""
    def make():
        from tests import calib_cases as cc
        from tests import calib_ref as cr
        from tests import projective_cases as pc
        if which == "edge":
            recs, h8, part = pc.edge_records()
            return dict(recs=recs, h8=h8, part=part)
        if which == "calib_edge":
            recs, h8 = cc.edge_records()
            return dict(recs=recs, h8=h8)
        s = pc.survey(which, 0.5)
        mix = lambda r: np.concatenate([r, r[:3]])
        recs = mix(s["recs"].copy())
        recs["accepted"][-3:] = 0
        recs = recs[np.random.default_rng(4).permutation(len(recs))]
        crecs = mix(cc.survey(which, 0.5).copy())
        crecs["accepted"][-3:] = 0
        crecs = crecs[np.random.default_rng(4).permutation(len(crecs))]
        return dict(recs=recs, w=s["w"], h=s["h"], start=s["start"], crecs=crecs, ch8=np.array([cr.start_state(r["H"], cc.CAM_START) for r in crecs]))
    return _pair_once(("lm", which), make)


def _compact(which, count):
    R = lm_records(which)["recs"][:count]

    def run(env, ctx):
        im = env.im
        d_in = _recs_dev(env, R)
        d_out = env.full((len(R), im.PAIR_RESULT.itemsize), 0xAB, env.torch.uint8)
        k = ctx.CompactAcceptedDev(d_in.data_ptr(), len(R), d_out.data_ptr())
        ctx.synchronize()
        got = d_out.cpu().numpy()
        assert (got[k:] == 0xAB).all()
        return [np.array([k]), got[:k]]
    kept = R[R["accepted"] != 0]
    return Step("compact accepted %s, %d records" % (which, count), run, lambda orc: [np.array([len(kept)]), _raw(kept).reshape(len(kept), -1)],
                dict(ag_res_compact=len(kept)), "compact %s %d" % (which, count))


def _moments(which, count):
    R = lm_records(which)["recs"][:count]

    def run(env, ctx):
        im = env.im
        d_m = _guarded(env, len(R), im.PAIR_MOMENTS.itemsize)
        ctx.PairMomentsDev(_recs_dev(env, R).data_ptr(), len(R), d_m.data_ptr())
        ctx.synchronize()
        return [_unguard(d_m, len(R))]

    def ref(orc):
        import imagemosaicing_amd as im
        return [_raw(im.pair_moments_host(R)).reshape(len(R), -1)]
    return Step("pair moments %s, %d records" % (which, len(R)), run, ref, dict(moments_records=len(R)), "moments %s %d" % (which, len(R)))


def _normal_blocks(count):
    E = lm_records("edge")

    def run(env, ctx):
        im = env.im
        d_b = _guarded(env, count, im.PAIR_NORMAL_BLOCK.itemsize)
        ctx.PairNormalBlocksDev(_recs_dev(env, E["recs"]).data_ptr(), count, E["h8"], E["part"], d_b.data_ptr())
        ctx.synchronize()
        return [_unguard(d_b, count)]

    def ref(orc):
        import imagemosaicing_amd as im
        want = _pair_once("normal blocks", lambda: im.pair_normal_blocks_host(E["recs"], E["h8"], E["part"]))
        return [_raw(want[:count]).reshape(count, -1)]
    return Step("pair normal blocks, %d records" % count, run, ref, dict(proj_blocks=count), "normal %d" % count)


def _calib_blocks(which, count):
    from tests import calib_cases as cc
    L = lm_records(which)
    recs, h8 = (L["recs"], L["h8"]) if which == "calib_edge" else (L["crecs"], L["ch8"])
    recs, h8 = recs[:count], h8[:count]

    def cam(im):
        return im.Camera(*(cc.CAM_TRUE[:4] + tuple(cc.THETA_TRUE)))

    def run(env, ctx):
        im = env.im
        d_b = _guarded(env, len(recs), im.PAIR_CALIB_BLOCK.itemsize)
        ctx.PairCalibBlocksDev(_recs_dev(env, recs).data_ptr(), len(recs), h8, cam(im), d_b.data_ptr())
        ctx.synchronize()
        return [_unguard(d_b, len(recs))]

    def ref(orc):
        import imagemosaicing_amd as im
        return [_raw(im.pair_calib_blocks_host(recs, h8, cam(im))).reshape(len(recs), -1)]
    return Step("pair calib blocks %s, %d records" % (which, len(recs)), run, ref, dict(calib_blocks=len(recs)), "calib blocks %s %d" % (which, len(recs)))


def _report_array(rep):
    return np.array([float(rep[k]) for k in sorted(rep)], np.float64).view(np.uint64)


def _projective_loop(which, prior):
    L = lm_records(which)

    def run(env, ctx):
        got, rep = ctx.GlobalProjectiveRefineDev(_recs_dev(env, L["recs"]).data_ptr(), len(L["recs"]), L["w"], L["h"], L["start"], params=env.im.projective_params(prior=prior))
        return [_raw(got), _report_array(rep)]

    def ref(orc):
        import imagemosaicing_amd as im
        want, rep = _pair_once(("projective", which, prior), lambda: im.global_projective_refine_results(L["recs"], L["w"], L["h"], L["start"], params=im.projective_params(prior=prior)))
        return [_raw(want), _report_array(rep)]
    kept = int((L["recs"]["accepted"] != 0).sum())
    return Step("projective refine %s" % which, run, ref, dict(proj_compact=len(L["recs"]), proj_blocks=kept), "projective " + which)


def _calib_loop(which, mask):
    from tests import calib_cases as cc
    L = lm_records(which)

    def run(env, ctx):
        got, rep = ctx.CalibrateLensDev(_recs_dev(env, L["crecs"]).data_ptr(), len(L["crecs"]), env.im.Camera(*cc.CAM_START), mask=mask)
        return [_raw(np.frombuffer(bytes(got), np.uint8)), _report_array(rep)]

    def ref(orc):
        import imagemosaicing_amd as im
        want, rep = _pair_once(("calibrate", which, mask), lambda: im.calibrate_lens_results(L["crecs"], im.Camera(*cc.CAM_START), mask=mask))
        return [_raw(np.frombuffer(bytes(want), np.uint8)), _report_array(rep)]
    kept = int((L["crecs"]["accepted"] != 0).sum())
    return Step("calibrate lens %s" % which, run, ref, dict(calib_compact=len(L["crecs"]), calib_blocks=kept), "calibrate " + which)


def pair_steps():
    """The two loops' reference is the host twin (global_projective_refine_results, calibrate_lens_results, pair_*_blocks_host), bit for bit;
    the CPU suites hold the twins to tests/projective_ref.py and tests/calib_ref.py."""
    from tests import verify_cases as vc
    return [
        _refine_ties("six", "device", 3, 2),                   # six records, up to 400 ties
        _refine_ties("three", "host", 3, 2),                   # the host form: tie_records, tie_outputs, tie_srcs
        _refine_ties("one", "in place", 3, 2),                 # one record of one tie
        _refine_ties("six", "in place", 4, 1),
        _residual_stats("six", 16, 16),                        # 6 frames, 17 x 17 nodes
        _residual_stats("two", 3, 2),                          # 2 frames, 4 x 3 nodes
        _local_register("six", 8, 6),
        _local_register("two", 3, 2),
        _undistort("sixteen 64 x 48", 64, 48, 16, in_place=False),
        _apply_warps("twenty mixed", [[(37, 29), (64, 48), (5, 7), (130, 9), (33, 29)][k % 5] for k in range(20)], 3, 2, in_place=True),
        _undistort("one 2 x 2", 2, 2, 1, in_place=True),
        _apply_warps("one 2 x 2", [(2, 2)], 1, 1, in_place=False),
        _undistort("sixteen 64 x 48, in place", 64, 48, 16, in_place=True),
        _pair_edges(257), _pair_edges(1),
        _pair_residuals(257), _pair_residuals(1),
        _pair_cycles("300 common neighbours", lambda: vc.translation_graph(300, err=(3.0, 4.0), seed=300)),
        _pair_cycles("special graph", vc.special_graph),
        _verify_pairs("grid36", 2, 10),                        # a large graph ...
        _verify_pairs("strip_adjacent", 2, 0),                 # ... before 11 pairs in a chain
        _guided("six", 257),
        _match_plain("six"),
        _guided("tiny", 1),                                    # one pair of 3 keypoints
        _screen(6), _screen(2),
        _compact("edge", 257),
        _normal_blocks(257),
        _projective_loop("grid16", 0.01),                      # 45 records into proj_compact
        _calib_blocks("calib_edge", 5),
        _calib_loop("grid16", 15),                             # finds the projective loop's ag_res_counts; 32 records into calib_compact
        _projective_loop("strip12", 0.0),                      # 14 records behind 45, and the calibration's counts
        _calib_loop("strip12", 3),                             # 14 behind 32
        _compact("edge", 3),
        _moments("grid16", 45), _moments("grid16", 1),
        _normal_blocks(1),
        _calib_blocks("grid16", 32),
        _calib_blocks("calib_edge", 1),
    ]
