"""GPU: the record family on ONE used context -- tie refinement (device, in place, host), the residual statistics, local registration and its
apply, lens undistortion, the verification kernels and loop, guided matching with a plain MatchPairsDev on the same features in between, the
descriptor screen, compaction, moments, the block entry points and the two LM loops (tests/used_context.py: pair_steps).

Every step is held, byte for byte, to its stage's own reference (tests/tie_refine_ref.py, local_warp_ref.py, undistort_ref.py, verify_ref.py,
guided_ref.py with the _pad word left out as in tests/test_gpu_guided.py, the composed oracle of tests/match_patterns.py, screen_ref.py) and to
the same call on a fresh context.  The reference of the two LM loops and of the block entry points is the host twin
(global_projective_refine_results, calibrate_lens_results, pair_normal_blocks_host, pair_calib_blocks_host, pair_moments_host), bit for bit;
the CPU suites already hold the twins to tests/projective_ref.py and tests/calib_ref.py.  The records and transforms VerifyPairsDev returns
come out of the host alignment and are held to verify_pairs_results, its decisions to tests/verify_ref.py.

The second test covers the pinned staging tables: two calls with different tables, enqueued behind a delay without a wait between them.
"""
import numpy as np
import pytest

from tests import used_context as uc

pytestmark = pytest.mark.gpu

# The delay enqueued in front of call 1, in ms.  Found on an MI355X by running _staged() at 1, 2, 5, 10, 20, 50 and 100 ms, three runs each: 1 ms is
# the shortest round figure at which event.query() was still false when call 1 returned, three runs in a row, for the entry point that
# does not wait by itself (PairEdgesDev).  The others were complete at every delay up to the 100 ms cap: see SELF_WAITING.
DELAY_MS = 1
# Entry points whose event was already complete when call 1 returned, at every delay from 1 to 100 ms, with the reason.  For these the delay
# shows nothing while the wait is there; with the wait taken out, call 1 returns at once and call 2 restages the table before call 1's copy
# has run, which the comparison of call 1 with its reference then shows.
_WAITS = "waits for the ctx stream (hipStreamSynchronize) before it overwrites its pinned staging table, at the start of every call: "
SELF_WAITING = {
    "RefineTiesDev": _WAITS + "tie_frames_host (csrc/tie_refine.hip, launch_ties)",
    "TieResidualStatsDev": _WAITS + "local_warp_geo_host (csrc/local_warp.hip)",
    "PairResidualsDev": _WAITS + "verify_*_host (csrc/verify.hip)",
    "PairNormalBlocksDev": _WAITS + "<prefix>_params_host (csrc/tie_blocks_dev.h)",
    "PairCalibBlocksDev": _WAITS + "<prefix>_params_host (csrc/tie_blocks_dev.h)",
    "GuidedSelectDev": "uploads its pair and guide table from a vector of its own and waits for that copy before the launch (csrc/guided.hip, guided_select)",
}


def test_records_on_one_used_context(oracle):
    import torch
    import imagemosaicing_amd as im
    env = uc.Env(torch, im)
    res = uc.run_steps(env, uc.pair_steps(), oracle)
    # the cases do what they were built for
    six = res["refine ties six, device"]
    assert six[3].size > 0 and (six[1].reshape(6, 400)[5] == 1).sum() > 300                   # 400 ties, most of them REFINED (status 1)
    assert res["guided select and match six, 257 pairs"][2].max() > 30 and res["guided select and match tiny, 1 pairs"][2].max() <= 3
    verdict = res["verify pairs grid36, 10 % wrong"][0]
    assert len(set(verdict.tolist())) >= 2                                                      # wrong pairs were found among the right ones
    assert res["compact accepted edge, 257 records"][0][0] == 214 and res["screen scores, 6 frames"][0].max() > 0


def _sleep_cycles_per_ms(torch, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        torch.cuda._sleep(1000)                                                                 # warm the kernel up
        a.record(stream)
        torch.cuda._sleep(20_000_000)
        b.record(stream)
    stream.synchronize()
    return 20_000_000 / a.elapsed_time(b)


def _delay(torch, stream, ms, per_ms):
    """a delay of about `ms` on the stream: torch.cuda._sleep where this build has it, otherwise a chain of large matmuls"""
    with torch.cuda.stream(stream):
        if per_ms:
            torch.cuda._sleep(int(ms * per_ms))
        else:
            x = torch.ones((4096, 4096), device="cuda")
            for _ in range(int(4 * ms)):
                x = (x @ x) * 1e-4


def staged_entries(env, oracle):
    """name -> (call(ctx, variant) enqueues on the ctx stream and returns the device tensors it writes, ref(variant) their bytes).  Variant 0
    and variant 1 differ in the table or parameter block the entry point stages through pinned memory.  Every device buffer is made here,
    before any delay is enqueued."""
    import imagemosaicing_amd as im
    torch = env.torch
    from tests import calib_cases as cc
    from tests import guided_cases as gc
    from tests import guided_ref as gr
    from tests import local_warp_ref as lr
    from tests import tie_refine_cases as tc
    from tests import tie_refine_ref as tr
    from tests import verify_cases as vc
    from tests import verify_ref as vr
    from tests.test_gpu_tie_refine import DevFrames
    out = {}

    def outputs(sizes):
        return [env.full((n,), 0xCD, torch.uint8) for n in sizes]

    # RefineTiesDev: the frame table (tie_frames_host) and the parameter block
    T = uc.tie_cases()
    s_imgs, s_recs, _ = tc.status_case()
    tie = [(T["six"], T["imgs"], dict(radius=3, search=2)), (s_recs, s_imgs, dict(radius=7, search=3))]
    tie_dev = [(uc._recs_dev(env, r), DevFrames(torch, i), outputs([len(r) * tr.PAIR_RESULT.itemsize, len(r) * 400, len(r) * 1600, len(r) * 64])) for r, i, _ in tie]

    def tie_call(ctx, v):
        d_in, fr, o = tie_dev[v]
        ctx.RefineTiesDev(d_in.data_ptr(), len(tie[v][0]), fr.ptrs, fr.w, fr.h, fr.ws, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), **tie[v][2])
        return o
    out["RefineTiesDev"] = (tie_call, lambda v: [uc._raw(a) for a in tr.refine_ties(tie[v][0], tie[v][1], **tie[v][2])])

    # TieResidualStatsDev: the frames' geometry (local_warp_geo_host) and the grid
    W = uc.warp_surveys()
    st = [(W["six"], dict(grid_x=8, grid_y=6)), (W["two"], dict(grid_x=3, grid_y=2))]
    st_dev = [(uc._recs_dev(env, s["rec"]), env.full((im.local_warp_stats_len(s["n"], p["grid_x"], p["grid_y"]),), 0x5a5a5a5a, torch.int64)) for s, p in st]

    def st_call(ctx, v):
        s, p = st[v]
        ctx.TieResidualStatsDev(st_dev[v][0].data_ptr(), len(s["rec"]), s["w"], s["h"], s["h9s"], st_dev[v][1].data_ptr(), **p)
        return [st_dev[v][1]]
    out["TieResidualStatsDev"] = (st_call, lambda v: [uc._raw(lr.stats(st[v][0]["rec"], st[v][0]["w"], st[v][0]["h"], st[v][0]["h9s"], **st[v][1]))])

    # PairEdgesDev / PairResidualsDev: the transforms and labels (verify_*_host)
    e_recs = vc.edge_records()
    h9, label = vc.edge_transforms()
    res_tab = [(h9, label), (np.ascontiguousarray(h9[::-1]), None)]
    d_e = uc._recs_dev(env, e_recs)
    res_out = [outputs([len(e_recs) * im.PAIR_RESIDUAL.itemsize]) for _ in range(2)]
    edge_n = [len(e_recs), 5]
    edge_out = [outputs([n * im.PAIR_EDGE.itemsize]) for n in edge_n]

    def res_call(ctx, v):
        ctx.PairResidualsDev(d_e.data_ptr(), len(e_recs), res_tab[v][0], res_tab[v][1], res_out[v][0].data_ptr())
        return res_out[v]

    def edge_call(ctx, v):
        ctx.PairEdgesDev(d_e.data_ptr(), edge_n[v], vc.EDGE_IMAGES, edge_out[v][0].data_ptr())
        return edge_out[v]
    out["PairResidualsDev"] = (res_call, lambda v: [uc._raw(vr.residuals(e_recs, *res_tab[v]))])
    out["PairEdgesDev"] = (edge_call, lambda v: [uc._raw(vr.edges(e_recs, vc.EDGE_IMAGES)[:edge_n[v]])])

    # PairNormalBlocksDev: the parameters and flags of the images (<prefix>_params_host)
    E = uc.lm_records("edge")
    nb_tab = [(E["h8"], E["part"]), (np.ascontiguousarray(E["h8"][::-1]), np.ascontiguousarray(E["part"][::-1]))]
    d_n = uc._recs_dev(env, E["recs"])
    nb_out = [outputs([len(E["recs"]) * im.PAIR_NORMAL_BLOCK.itemsize]) for _ in range(2)]

    def nb_call(ctx, v):
        ctx.PairNormalBlocksDev(d_n.data_ptr(), len(E["recs"]), nb_tab[v][0], nb_tab[v][1], nb_out[v][0].data_ptr())
        return nb_out[v]
    out["PairNormalBlocksDev"] = (nb_call, lambda v: [uc._raw(im.pair_normal_blocks_host(E["recs"], *nb_tab[v]))])

    # PairCalibBlocksDev: the per-record states and the camera
    Cc = uc.lm_records("calib_edge")
    cams = [im.Camera(*(cc.CAM_TRUE[:4] + tuple(cc.THETA_TRUE))), im.Camera(*(cc.CAM_TRUE[:4] + (-0.1, 0.02, 0.001, -0.002, 0.01)))]
    cb_h8 = [Cc["h8"], np.ascontiguousarray(Cc["h8"] * 1.001)]
    d_c = uc._recs_dev(env, Cc["recs"])
    cb_out = [outputs([len(Cc["recs"]) * im.PAIR_CALIB_BLOCK.itemsize]) for _ in range(2)]

    def cb_call(ctx, v):
        ctx.PairCalibBlocksDev(d_c.data_ptr(), len(Cc["recs"]), cb_h8[v], cams[v], cb_out[v][0].data_ptr())
        return cb_out[v]
    out["PairCalibBlocksDev"] = (cb_call, lambda v: [uc._raw(im.pair_calib_blocks_host(Cc["recs"], cb_h8[v], cams[v]))])

    # GuidedSelectDev: the pair and guide table
    scenes = uc.guided_scenes("six")
    order = [[(5 * p + p // 7) % len(scenes) for p in range(257)], [(3 * p + 1) % len(scenes) for p in range(40)]]
    gs_out = [outputs([len(o) * 400 * 12, len(o) * 400 * 12, len(o) * 4, len(o) * 400 * 4]) for o in order]

    def gs_call(ctx, v):
        pairs, guides = [(2 * k, 2 * k + 1) for k in order[v]], [scenes[k]["G"] for k in order[v]]
        o = gs_out[v]
        ctx.GuidedSelectDev(pairs, guides, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr())
        return o

    def gs_ref(v):
        sel = [gr.lists_400(*gc.ref_select(s)) for s in scenes]
        nsel = np.array([len(gc.ref_select(s)[0]) for s in scenes], np.int32)
        return [uc._raw(np.stack([sel[k][0] for k in order[v]])), uc._raw(np.stack([sel[k][1] for k in order[v]])), uc._raw(nsel[order[v]]),
                uc._raw(np.stack([sel[k][2] for k in order[v]]))]
    out["GuidedSelectDev"] = (gs_call, gs_ref)
    torch.cuda.synchronize()
    return out, scenes


def _staged(env, oracle, delay_ms):
    """{entry point: (event complete when call 1 returned, first difference of call 1 from its reference, of call 2)}: on one context set to
    a torch stream, a delay, an event, call 1 and call 2 with another table, no host synchronisation in between"""
    from tests.test_gpu_guided import _install_case
    torch, im = env.torch, env.im
    entries, scenes = staged_entries(env, oracle)
    stream = torch.cuda.Stream()
    per_ms = _sleep_cycles_per_ms(torch, stream) if hasattr(torch.cuda, "_sleep") else 0
    ctx = im.Context(0)
    for k, s in enumerate(scenes):
        _install_case(ctx, k, s)
    ctx.synchronize()
    ctx.set_stream(stream.cuda_stream)
    seen = {}
    try:
        for name, (call, ref) in entries.items():
            stream.synchronize()
            event = torch.cuda.Event()
            _delay(torch, stream, delay_ms, per_ms)
            event.record(stream)
            first = call(ctx, 0)
            done = event.query()
            second = call(ctx, 1)
            stream.synchronize()
            got = [[uc._raw(t.cpu().numpy()) for t in first], [uc._raw(t.cpu().numpy()) for t in second]]
            seen[name] = (done, uc.first_difference(got[0], ref(0)), uc.first_difference(got[1], ref(1)))
    finally:
        ctx.set_stream(None)
        ctx.close()
    return seen


def test_staging_tables_survive_a_second_call_without_a_wait(oracle):
    """RefineTiesDev, TieResidualStatsDev, PairEdgesDev / PairResidualsDev, PairNormalBlocksDev, PairCalibBlocksDev and GuidedSelectDev return
    before their work has run and stage a table through pinned memory.  Call 2 restages another table while call 1 is still queued behind the
    delay; both results must be their references'."""
    import torch
    import imagemosaicing_amd as im
    seen = _staged(uc.Env(torch, im), oracle, DELAY_MS)
    assert len(seen) == 7
    for name, (done, d1, d2) in seen.items():
        assert d1 is None, "%s, call 1: %s" % (name, d1)
        assert d2 is None, "%s, call 2: %s" % (name, d2)
        if name not in SELF_WAITING:
            assert not done, name + ": the event was complete when call 1 returned: the delay is too short, or the entry point waits by itself"
    assert set(SELF_WAITING) < set(seen) and set(seen) - set(SELF_WAITING) == {"PairEdgesDev"}
