"""CPU: what imagemosaicing_amd/capi.py hands to the C ABI, call by call, against a recording stand-in for the library.

The stand-in logs every call (function name and each argument by kind and content) and returns 0; only mi355_default_*, mi355_last_error
and the three host-only layout functions the Into / blended forms size their outputs with are also run in the real library, which builds
and loads without a GPU.  tests/golden/capi_calls.json holds the log, the value every call returned, the public surface (names,
signatures, docstring checksums) and which wrapper raises on which return code.  It was written from the binding as it stood BEFORE the
helpers of this file's subject were shared (`python -m tests.test_capi_calls` at that commit), so it records the behaviour to keep, never
the code under test: regenerate it only from a binding known to be right."""
import ctypes as C
import inspect
import json
import os
import zlib
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "capi_calls.json")
_BYREF = type(C.byref(C.c_int()))
_LAYOUTS = ("mi355_mosaic_layout", "mi355_blend_layout", "mi355_overview_layout")

# methods the stand-in cannot drive (at most three)
SKIP = {"MosaicBlendedDev": "allocates its canvas as a CUDA tensor"}


def _crc(b):
    return "%08x" % (zlib.crc32(bytes(b)) & 0xffffffff)


def _nd(a):
    return ["nd", a.dtype.str, list(a.shape), _crc(np.ascontiguousarray(a).tobytes())]


def _addr(v):
    return None if not v else (int(v) if int(v) < 4096 else "ptr")


class Recorder:
    """stands in for the CDLL: L.mi355_x(...) appends [name, arg, ...] to .log and returns .rc"""

    def __init__(self, real):
        self.real, self.log, self.rc, self.arrays = real, [], 0, {}

    def arg(self, a):
        if a is None:
            return None
        if isinstance(a, (bool, int)):
            return int(a)
        if isinstance(a, np.integer):
            return ["npint", int(a)]
        if isinstance(a, bytes):
            return ["bytes", a.decode()]
        if isinstance(a, (C.c_float, C.c_double, C.c_uint32, C.c_int64)):
            return [type(a).__name__, a.value]
        if isinstance(a, _BYREF):
            x = a._obj
            return ["byref", type(x).__name__] + ([bytes(x).hex()] if isinstance(x, C.Structure) else [])
        if isinstance(a, C.Array):
            if a._type_ is C.c_void_p:
                return ["ptrs", len(a), [_addr(v) for v in a]]
            return ["array", a._type_.__name__, len(a), _crc(a)]
        if isinstance(a, C.c_void_p):
            if a.value in self.arrays:
                return _nd(self.arrays[a.value])
            return ["p", _addr(a.value)]
        if isinstance(a, C._Pointer):
            return ["pointer", type(a).__name__, bool(a)]
        if isinstance(a, C._CFuncPtr):
            return "callback"
        return ["?", type(a).__name__]

    def __getattr__(self, name):
        if not name.startswith("mi355_"):
            raise AttributeError(name)
        if name.startswith("mi355_default_") or (name == "mi355_last_error" and self.rc == 0):
            return getattr(self.real, name)

        def call(*args):
            self.log.append([name] + [self.arg(a) for a in args])
            if name in _LAYOUTS and self.rc == 0:
                getattr(self.real, name)(*args)          # what it refuses (overview levels = 0) leaves its outputs zero
                return 0
            if name == "mi355_last_error":
                return b"recorded error"
            return self.rc
        return call


def _ret(v):
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, bytes):
        return ["bytes", _crc(v)]
    if isinstance(v, np.ndarray):
        return _nd(v)
    if isinstance(v, np.generic):
        return ["npscalar", v.dtype.str, _crc(v.tobytes())]
    if isinstance(v, (tuple, list)):
        return [_ret(x) for x in v]
    if isinstance(v, dict):
        return {k: _ret(x) for k, x in sorted(v.items())}
    if isinstance(v, C.Structure):
        return ["struct", type(v).__name__, bytes(v).hex()]
    return ["?", type(v).__name__]


def _run(rec, name, fn):
    rec.log = []
    rec.arrays.clear()
    try:
        out = {"call": name, "ret": _ret(fn())}
    except Exception as e:                                      # the checks before a call are part of the behaviour
        out = {"call": name, "raises": [type(e).__name__, str(e)]}
    out["lib"] = rec.log
    return out


@pytest.fixture(scope="module")
def capi():
    from imagemosaicing_amd import build
    build.build()
    from imagemosaicing_amd import capi
    return capi


def _install(capi, mp):
    """the recorder as the library every load_library() returns, and _p remembering the array behind each address"""
    rec = Recorder(capi.load_library())
    mp.setattr(capi, "_LIB", rec)
    real_p = capi._p

    def p(a):
        r = real_p(a)
        if a is not None:
            rec.arrays[r.value] = a            # a strong reference: no other array takes the address while the wrapper runs
        return r
    mp.setattr(capi, "_p", p)
    return rec


def _inputs(capi):
    rng = np.random.default_rng(5)
    imgs = [rng.integers(0, 256, (6, 8, 3), dtype=np.uint8) for _ in range(2)]
    h9s = np.array([[1, 0, 0, 0, 1, 0, 0, 0, 1], [1, 0, 3, 0, 1, 2, 0, 0, 1]], np.float32)
    res = np.zeros(2, capi.PAIR_RESULT)
    res["i"], res["j"], res["n_in"], res["accepted"] = [0, 0], [1, 1], [5, 3], [1, 0]
    return dict(imgs=imgs, h9s=h9s, w=[8, 8], h=[6, 6], ws=[24, 24], d=[16, 32], res=res, pairs=[(0, 1)],
                geom=[(8, 6, 24), (8, 6, 24)], cam=capi.Camera(100, 100, 4, 3, 0.1, 0.01, 0, 0, 0))


def context_calls(capi, x):
    """(label, callable(ctx)): every Context method, once per variant of its optional inputs and outputs"""
    I, H, W, HH, WS, D, G = x["imgs"], x["h9s"], x["w"], x["h"], x["ws"], x["d"], x["geom"]
    geo = (D, W, HH, WS, H)
    kp, desc = np.zeros(3, capi.KEYPOINT), np.ones((3, 128), np.float32)
    xy = np.arange(8, dtype=np.float32).reshape(4, 2)
    sf = np.zeros(5, capi.SFPOINT)
    sf["x"] = np.arange(5)
    out12 = np.zeros((12, 40), np.uint8)
    h8 = np.arange(16, dtype=np.float64).reshape(2, 8)
    calls = [
        ("set_stream", lambda c: c.set_stream(0)), ("set_stream", lambda c: c.set_stream(64)), ("synchronize", lambda c: c.synchronize()),
        ("set_option", lambda c: c.set_option("keep_frames", 1)), ("set_option", lambda c: (c.set_option("nfeatures", 100), c.params.nfeatures)),
        ("profile_enable", lambda c: c.profile_enable()), ("profile_only", lambda c: c.profile_only()),
        ("profile_only", lambda c: c.profile_only("sift")), ("profile_reset", lambda c: c.profile_reset()),
        ("profile_get", lambda c: c.profile_get("sift")),
        ("SiftExtract", lambda c: c.SiftExtract(0, I[0])), ("SiftExtract", lambda c: c.SiftExtract(1, I[1], max_kp=16)),
        ("SiftExtractHost", lambda c: c.SiftExtractHost(1, I[1])),
        ("SiftExtractDev", lambda c: c.SiftExtractDev(0, 16, 8, 6, 24)), ("SiftExtractDev", lambda c: c.SiftExtractDev(1, 32, 8, 6, 24, want_count=True)),
        ("GetFeatures", lambda c: c.GetFeatures(0, 8)), ("SetFeatures", lambda c: c.SetFeatures(1, kp, desc, 8, 6)),
        ("DropFeatures", lambda c: c.DropFeatures()), ("DropFeatures", lambda c: c.DropFeatures(1)),
        ("MatchPairs", lambda c: c.MatchPairs(x["pairs"])), ("MatchPairs", lambda c: c.MatchPairs([0, 1, 1, 2], 3.0, 7)),
        ("MatchPairsDev", lambda c: c.MatchPairsDev(x["pairs"], 48)), ("MatchPairsDev", lambda c: c.MatchPairsDev(x["pairs"], 48, 3.0, 7)),
        ("ScreenPairs", lambda c: c.ScreenPairs([0, 1])),
        ("ScreenPairs", lambda c: c.ScreenPairs([0, 1], window=3, top_k=8, partners=2, min_score=3, ratio_pct=70, rank=1, world=2, return_scores=True)),
        ("ScreenScoresDev", lambda c: c.ScreenScoresDev([0, 1], 48)), ("ScreenScoresDev", lambda c: c.ScreenScoresDev([0, 1], 48, top_k=8, partners=1)),
        ("BFMatch", lambda c: c.BFMatch(0, 1, max_matches=4)), ("BFMatch", lambda c: c.BFMatch(0, 1, sorted_=False, max_matches=4)),
        ("SelectMatchPairs", lambda c: c.SelectMatchPairs(np.array([[0, 1], [2, 3]]), xy, xy + 1, 2, 8, 6)),
        ("SelectMatchPairs", lambda c: c.SelectMatchPairs(np.zeros(2, capi.DMATCH), xy, xy + 1, 2, 8, 6, gridX=2, gridY=1)),
        ("Ransac2D", lambda c: c.Ransac2D(sf, sf)), ("Ransac2D", lambda c: c.Ransac2D(sf, sf, 2.5, 10, 7)),
        ("ImageProjectionTransform", lambda c: c.ImageProjectionTransform(I[0], H[1])),
        ("ImageProjectionTransform", lambda c: c.ImageProjectionTransform(I[0][:, :, 0], H[1])),
        ("MosaicImagesRefined", lambda c: c.MosaicImagesRefined(I, H)), ("MosaicImagesRefined", lambda c: c.MosaicImagesRefined(I, H, want_pixels=False)),
        ("MosaicImagesRefinedDev", lambda c: c.MosaicImagesRefinedDev(D, W, HH, WS, H, 48, 11, 8, 36)),
        ("MosaicImagesRefinedDev", lambda c: c.MosaicImagesRefinedDev([16, 0], W, HH, WS, H, 48, 11, 8, 36, row0=2, rows=3)),
        ("SurfExtract", lambda c: c.SurfExtract(0, I[0], max_kp=8)), ("SurfExtract", lambda c: c.SurfExtract(0, I[0], hessian=20.0, max_kp=8)),
        ("SurfMatchPairs", lambda c: c.SurfMatchPairs(x["pairs"])),
        ("SurfMatchPairs", lambda c: c.SurfMatchPairs(x["pairs"], 3.0, 7, match_dist=0.4, max_features=100, min_inliers=9)),
        ("PackFeaturesDev", lambda c: c.PackFeaturesDev([0, 1], 48)), ("InstallFeaturesDev", lambda c: c.InstallFeaturesDev(np.zeros(2, capi.FEATURE_HEADER), 48)),
        ("FeatureChunkCount", lambda c: c.FeatureChunkCount([0, 1])),
        ("PackFeatureChunksDev", lambda c: c.PackFeatureChunksDev([0, 1], 48, 4)), ("PackFeatureChunksDev", lambda c: c.PackFeatureChunksDev([0, 1], 0, 0)),
        ("InstallFeatureChunksDev", lambda c: c.InstallFeatureChunksDev(np.zeros(2, capi.FEATURE_CHUNK_HEADER), 48)),
        ("InstallFeatureChunksDev", lambda c: c.InstallFeatureChunksDev(np.zeros(0, capi.FEATURE_CHUNK_HEADER), 0)),
        ("CompactAcceptedDev", lambda c: c.CompactAcceptedDev(16, 2, 32)), ("last_sift_counters", lambda c: c.last_sift_counters()),
        ("CommInit", lambda c: c.CommInit(bytes(range(128)), 0, 1)), ("CommDestroy", lambda c: c.CommDestroy()), ("CommInfo", lambda c: c.CommInfo()),
        ("AllGatherFeatures", lambda c: c.AllGatherFeatures([0, 1], 4)),
        ("AllGatherFeatureChunks", lambda c: c.AllGatherFeatureChunks([0, 1])), ("AllGatherFeatureChunks", lambda c: c.AllGatherFeatureChunks([0], install_own=True)),
        ("AllGatherResults", lambda c: c.AllGatherResults(16, 2)),
        ("AllGatherResults", lambda c: c.AllGatherResults(16, 2, accepted_only=False, root=0, copy=False, wait=False)),
        ("AllGatherResults", lambda c: c.AllGatherResults(16, 2, wait=False)),
        ("PairMomentsDev", lambda c: c.PairMomentsDev(16, 2, 32)), ("PairNormalBlocksDev", lambda c: c.PairNormalBlocksDev(16, 2, h8, [1, 2], 32)),
        ("PairNormalBlocksDev", lambda c: c.PairNormalBlocksDev(16, 2, h8, [1], 32)),
        ("GlobalProjectiveRefineDev", lambda c: c.GlobalProjectiveRefineDev(16, 2, W, HH, np.zeros(2, capi.IMAGE_TRANSFORM))),
        ("GlobalProjectiveRefineDev", lambda c: c.GlobalProjectiveRefineDev(0, 0, W, HH, np.zeros(2, capi.IMAGE_TRANSFORM), fixed=[1, 0], label=[1, 1],
                                                                            params=capi.projective_params(max_iters=3, prior=0.5))),
        ("PairCalibBlocksDev", lambda c: c.PairCalibBlocksDev(16, 2, h8, x["cam"], 32)),
        ("PairCalibBlocksDev", lambda c: c.PairCalibBlocksDev(None, 0, None, None, 0, min_ties=4)),
        ("CalibrateLensDev", lambda c: c.CalibrateLensDev(16, 2, x["cam"])), ("CalibrateLensDev", lambda c: c.CalibrateLensDev(0, 0, None, max_iters=5, mask=3)),
        ("CalibrateLensDev", lambda c: c.CalibrateLensDev(16, 2, x["cam"], params=capi.calib_params(min_ties=8, lambda0=0.5))),
        ("RefineTiesDev", lambda c: c.RefineTiesDev(16, 2, D, W, HH, WS, 32)),
        ("RefineTiesDev", lambda c: c.RefineTiesDev(16, 2, [0, None], W, HH, WS, 16, d_status=48, d_ncc2=64, d_report=80, radius=5, min_ncc=0.5)),
        ("RefineTiesDev", lambda c: c.RefineTiesDev(16, 2, D, W, HH, WS, 32, params=capi.tie_params(search=2))),
        ("RefineTies", lambda c: c.RefineTies(x["res"], I)), ("RefineTies", lambda c: c.RefineTies(x["res"], None, img_ids=[0, 1], geom=G, drop_mask=3)),
        ("RefineTies", lambda c: c.RefineTies(x["res"], [I[0], None], img_ids=[-1, 1], params=capi.tie_params(radius=4))),
        ("AllGatherMoments", lambda c: c.AllGatherMoments(16, 2)), ("AllGatherMoments", lambda c: c.AllGatherMoments(16, 2, copy=False)),
        ("StripeCover", lambda c: c.StripeCover(W, HH, H, 0, 4)), ("StripeCover", lambda c: c.StripeCover(W, HH, H, 1, 3, exact=True)),
        ("StripeCover", lambda c: c.StripeCover(W, HH, H, 1, 3, blended=True, keep=[1, 0], band=3)),
        ("ExchangeFrames", lambda c: c.ExchangeFrames([16, 0], HH, WS, [1, 1])),
        ("ExchangeFrames", lambda c: c.ExchangeFrames([None, 32], HH, WS, [[1, 0], [0, 1]], owner=[0, 1], own_through_rccl=True)),
        ("SynthFrameDev", lambda c: c.SynthFrameDev(16, 8, 6, 24, [1, 0, 0, 0, 1, 0], 3, 4)),
        ("SynthFrameDev", lambda c: c.SynthFrameDev(16, 8, 6, 24, [1, 0, 0, 0, 1, 0], 3, 4, gain=1.5, noise=0.0)),
        ("ChipsAndMasks", lambda c: c.ChipsAndMasks(I, H)), ("ChipsAndMasks", lambda c: c.ChipsAndMasks(I, H, keep=[1, 0], find_masks=False)),
        ("MultiBandBlend", lambda c: c.MultiBandBlend(np.zeros(1, capi.CHIPINFO), [np.ones((4, 12), np.uint8)], [np.ones((4, 4), np.uint8)], 11, 8)),
        ("MultiBandBlend", lambda c: c.MultiBandBlend(np.zeros(0, capi.CHIPINFO), [], [], 11, 8, band=3)),
        ("MosaicBlended", lambda c: c.MosaicBlended(I, H)), ("MosaicBlended", lambda c: c.MosaicBlended(I, H, keep=[1, 1], band=3)),
        ("GainStatsDev", lambda c: c.GainStatsDev(*geo, x["pairs"])), ("GainStatsDev", lambda c: c.GainStatsDev([16, None], W, HH, WS, H, [], step=4)),
        ("ApplyGainsDev", lambda c: c.ApplyGainsDev(D, [48, 0], W, HH, WS, np.ones((2, 3)))),
        ("GainCompensateDev", lambda c: c.GainCompensateDev(*geo, x["pairs"])), ("GainCompensateDev", lambda c: c.GainCompensateDev(*geo, x["pairs"], sigma_n=5, step=4)),
        ("GainCompensateDev", lambda c: c.GainCompensateDev(*geo, x["pairs"], params=capi.gain_params(channels=1))),
        ("SharpStatsDev", lambda c: c.SharpStatsDev(*geo, x["pairs"])), ("SharpStatsDev", lambda c: c.SharpStatsDev(*geo, x["pairs"], step=4, frames=False)),
        ("SharpnessDev", lambda c: c.SharpnessDev(*geo, x["pairs"])), ("SharpnessDev", lambda c: c.SharpnessDev(*geo, x["pairs"], prior=0.1, step=2)),
        ("SharpnessDev", lambda c: c.SharpnessDev(*geo, x["pairs"], params=capi.sharp_params(blur_ratio=0.5))),
        ("CoverStatsDev", lambda c: c.CoverStatsDev(W, HH, H)), ("CoverStatsDev", lambda c: c.CoverStatsDev(W, HH, H, keep=[1, 0], step=2)),
        ("CoverStatsDev", lambda c: c.CoverStatsDev(W, HH, H, keep=[1])),
        ("CoverSelectDev", lambda c: c.CoverSelectDev(W, HH, H)),
        ("CoverSelectDev", lambda c: c.CoverSelectDev(W, HH, H, order=[1, 0], pairs=x["pairs"], keep=[1, 1], final=True, min_depth=2, max_loss=5)),
        ("CoverSelectDev", lambda c: c.CoverSelectDev(W, HH, H, params=capi.cover_params(step=2))),
        ("BlockGainStatsDev", lambda c: c.BlockGainStatsDev(*geo, x["pairs"])), ("BlockGainStatsDev", lambda c: c.BlockGainStatsDev(*geo, x["pairs"], step=2, grid_x=3, grid_y=2)),
        ("ApplyBlockGainsDev", lambda c: c.ApplyBlockGainsDev(D, D, W, HH, WS, np.ones((2, 2, 3, 3)))),
        ("ApplyBlockGainsDev", lambda c: c.ApplyBlockGainsDev(D, D, W, HH, WS, np.ones((2, 3)))),
        ("BlockGainCompensateDev", lambda c: c.BlockGainCompensateDev(*geo, x["pairs"])),
        ("BlockGainCompensateDev", lambda c: c.BlockGainCompensateDev(*geo, x["pairs"], grid_x=3, grid_y=2, smooth=1)),
        ("BlockGainCompensateDev", lambda c: c.BlockGainCompensateDev(*geo, x["pairs"], params=capi.block_gain_params(sigma_g=0.2))),
        ("MosaicFeathered", lambda c: c.MosaicFeathered(I, H)), ("MosaicFeathered", lambda c: c.MosaicFeathered(I, H, want_pixels=False, ramp=3)),
        ("MosaicFeathered", lambda c: c.MosaicFeathered(I, H, params=capi.feather_params(ramp=2))),
        ("MosaicFeatheredDev", lambda c: c.MosaicFeatheredDev(*geo, 48, 11, 8, 36)),
        ("MosaicFeatheredDev", lambda c: c.MosaicFeatheredDev([16, None], W, HH, WS, H, 48, 11, 8, 36, row0=2, rows=3, ramp=3)),
        ("MosaicFeatheredDev", lambda c: c.MosaicFeatheredDev(*geo, 48, 11, 8, 36, params=capi.feather_params(ramp=2))),
        ("MosaicFeatheredInto", lambda c: c.MosaicFeatheredInto(I, None, H)), ("MosaicFeatheredInto", lambda c: c.MosaicFeatheredInto(None, [0, 1], H, geom=G, ramp=3)),
        ("MosaicFeatheredInto", lambda c: c.MosaicFeatheredInto(I, None, H, out=out12, pitch=40, params=capi.feather_params(ramp=2))),
        ("MosaicSeamline", lambda c: c.MosaicSeamline(I, H)), ("MosaicSeamline", lambda c: c.MosaicSeamline(I, H, want_owner=True, ramp=3)),
        ("MosaicSeamline", lambda c: c.MosaicSeamline(I, H, params=capi.seamline_params(ramp=2))),
        ("MosaicSeamlineDev", lambda c: c.MosaicSeamlineDev(*geo, 48, 11, 8, 36)),
        ("MosaicSeamlineDev", lambda c: c.MosaicSeamlineDev(None, W, HH, None, H, 0, 11, 8, 36, row0=2, rows=3, d_owner=64, d_count=80, ramp=3)),
        ("MosaicSeamlineDev", lambda c: c.MosaicSeamlineDev([16, 0], W, HH, WS, H, 48, 11, 8, 36, d_owner=64, params=capi.seamline_params(ramp=2))),
        ("MosaicSeamlineInto", lambda c: c.MosaicSeamlineInto(I, None, H)), ("MosaicSeamlineInto", lambda c: c.MosaicSeamlineInto(None, [0, 1], H, geom=G, ramp=3)),
        ("MosaicSeamlineInto", lambda c: c.MosaicSeamlineInto(I, None, H, out=out12, pitch=40, params=capi.seamline_params(ramp=2))),
        ("SeamlineCover", lambda c: c.SeamlineCover(W, HH, H)), ("SeamlineCover", lambda c: c.SeamlineCover(W, HH, H, row0=1, rows=3, ramp=3)),
        ("SeamlineCover", lambda c: c.SeamlineCover(W, HH, H, params=capi.seamline_params(ramp=2))),
        ("SeamCandidatesDev", lambda c: c.SeamCandidatesDev(*geo, 48, 2, 1)), ("SeamCandidatesDev", lambda c: c.SeamCandidatesDev(*geo, 48, 2, 1, level=2)),
        ("SeamCandidatesDev", lambda c: c.SeamCandidatesDev(None, W, HH, None, H, 0, 2, 1, params=capi.seamcut_params(depth=2))),
        ("SeamLabelsDev", lambda c: c.SeamLabelsDev(48, 2, 1, 64)), ("SeamLabelsDev", lambda c: c.SeamLabelsDev(48, 2, 1, 64, seam_penalty=3)),
        ("SeamLabelsDev", lambda c: c.SeamLabelsDev(0, 2, 1, 0, params=capi.seamcut_params(miss_cost=9))),
        ("SeamCellsDev", lambda c: c.SeamCellsDev(*geo, 64, 2, 1)), ("SeamCellsDev", lambda c: c.SeamCellsDev(*geo, 64, 2, 1, data_weight=2)),
        ("SeamCellsDev", lambda c: c.SeamCellsDev(*geo, 64, 2, 1, params=capi.seamcut_params(diff_weight=3))),
        ("MosaicSeamCutDev", lambda c: c.MosaicSeamCutDev(*geo, 48, 11, 8, 36)),
        ("MosaicSeamCutDev", lambda c: c.MosaicSeamCutDev(None, W, HH, None, H, 0, 11, 8, 36, row0=2, rows=3, d_cells=96, d_owner=64, d_count=80, level=2)),
        ("MosaicSeamCutDev", lambda c: c.MosaicSeamCutDev([16, 0], W, HH, WS, H, 48, 11, 8, 36, d_cells=96, params=capi.seamcut_params(ramp=2))),
        ("MosaicSeamCut", lambda c: c.MosaicSeamCut(I, H)), ("MosaicSeamCut", lambda c: c.MosaicSeamCut(I, H, want_owner=True, level=2)),
        ("MosaicSeamCut", lambda c: c.MosaicSeamCut(I, H, params=capi.seamcut_params(ramp=2))),
        ("MosaicSeamCutInto", lambda c: c.MosaicSeamCutInto(I, None, H)), ("MosaicSeamCutInto", lambda c: c.MosaicSeamCutInto(None, [0, 1], H, geom=G, level=2)),
        ("MosaicSeamCutInto", lambda c: c.MosaicSeamCutInto(I, None, H, out=out12, pitch=40, params=capi.seamcut_params(ramp=2))),
        ("SeamCutCover", lambda c: c.SeamCutCover(W, HH, H, 96)), ("SeamCutCover", lambda c: c.SeamCutCover(W, HH, H, 0, row0=1, rows=3, level=2)),
        ("SeamCutCover", lambda c: c.SeamCutCover(W, HH, H, 96, params=capi.seamcut_params(ramp=2))),
        ("BlendSeamCellsDev", lambda c: c.BlendSeamCellsDev(*geo, 64, 2, 1)),
        ("BlendSeamCellsDev", lambda c: c.BlendSeamCellsDev(*geo, 64, 2, 1, keep=[1, 1], d_cand=48, level=2)),
        ("BlendSeamCellsDev", lambda c: c.BlendSeamCellsDev(*geo, 64, 2, 1, params=capi.seamcut_params(ramp=2))),
        ("ChipsAndMasksSeam", lambda c: c.ChipsAndMasksSeam(I, H)),
        ("ChipsAndMasksSeam", lambda c: c.ChipsAndMasksSeam(I, H, keep=[1, 1], cells=np.ones((1, 2), np.uint16), level=2)),
        ("ChipsAndMasksSeam", lambda c: c.ChipsAndMasksSeam(I, H, params=capi.seamcut_params(ramp=2))),
        ("MosaicBlendedSeamDev", lambda c: c.MosaicBlendedSeamDev(*geo, 48, 11, 8, 36)),
        ("MosaicBlendedSeamDev", lambda c: c.MosaicBlendedSeamDev(*geo, 48, 11, 8, 36, keep=[1, 1], band=3, d_cells=96, gw=2, gh=1, level=2)),
        ("MosaicBlendedSeamDev", lambda c: c.MosaicBlendedSeamDev(*geo, 48, 11, 8, 36, params=capi.seamcut_params(ramp=2))),
        ("MosaicBlendedSeam", lambda c: c.MosaicBlendedSeam(I, H)), ("MosaicBlendedSeam", lambda c: c.MosaicBlendedSeam(I, H, keep=[1, 1], band=3, level=2)),
        ("MosaicBlendedSeam", lambda c: c.MosaicBlendedSeam(I, H, params=capi.seamcut_params(ramp=2))),
        ("MosaicBlendedSeamInto", lambda c: c.MosaicBlendedSeamInto(I, None, H)),
        ("MosaicBlendedSeamInto", lambda c: c.MosaicBlendedSeamInto(None, [0, 1], H, keep=[1, 1], band=3, geom=G, level=2)),
        ("MosaicBlendedSeamInto", lambda c: c.MosaicBlendedSeamInto(I, None, H, out=np.zeros((40, 64), np.uint8), pitch=64, params=capi.seamcut_params(ramp=2))),
        ("MosaicMedian", lambda c: c.MosaicMedian(I, H)), ("MosaicMedian", lambda c: c.MosaicMedian(I, H, want_spread=True, depth=3)),
        ("MosaicMedian", lambda c: c.MosaicMedian(I, H, params=capi.median_params(ramp=2))),
        ("MosaicMedianDev", lambda c: c.MosaicMedianDev(*geo, 48, 11, 8, 36)),
        ("MosaicMedianDev", lambda c: c.MosaicMedianDev(None, W, HH, None, H, 0, 11, 8, 36, row0=2, rows=3, d_spread=0, d_count=80, depth=3)),
        ("MosaicMedianDev", lambda c: c.MosaicMedianDev([16, 0], W, HH, WS, H, 48, 11, 8, 36, d_spread=64, params=capi.median_params(ramp=2))),
        ("MosaicMedianInto", lambda c: c.MosaicMedianInto(I, None, H)), ("MosaicMedianInto", lambda c: c.MosaicMedianInto(None, [0, 1], H, geom=G, depth=3)),
        ("MosaicMedianInto", lambda c: c.MosaicMedianInto(I, None, H, out=out12, pitch=40, params=capi.median_params(ramp=2))),
        ("MedianCover", lambda c: c.MedianCover(W, HH, H)), ("MedianCover", lambda c: c.MedianCover(W, HH, H, row0=1, rows=3, depth=3)),
        ("MedianCover", lambda c: c.MedianCover(W, HH, H, params=capi.median_params(ramp=2))),
        ("UndistortFramesDev", lambda c: c.UndistortFramesDev(D, [48, 64], W, HH, WS, [32, 32], x["cam"])),
        ("UndistortFramesDev", lambda c: c.UndistortFramesDev(D, D, W, HH, WS, WS, x["cam"], out_fx=90.0, fill=1)),
        ("UndistortFramesDev", lambda c: c.UndistortFramesDev(D, [48], W, HH, WS, WS, x["cam"], params=capi.undistort_params(fill=2))),
        ("UndistortImage", lambda c: c.UndistortImage(I[0], x["cam"])), ("UndistortImage", lambda c: c.UndistortImage(I[0], x["cam"], out=I[0].copy(), out_cx=3.5)),
        ("UndistortImage", lambda c: c.UndistortImage(I[0][:, :, 0], x["cam"])),
        ("UndistortImage", lambda c: c.UndistortImage(I[0], x["cam"], params=capi.undistort_params(fill=2), out=np.zeros((6, 8), np.uint8))),
        ("TieResidualStatsDev", lambda c: c.TieResidualStatsDev(16, 2, W, HH, H, 48)),
        ("TieResidualStatsDev", lambda c: c.TieResidualStatsDev(0, 0, W, HH, H, 0, grid_x=3, max_shift=2.5)),
        ("TieResidualStatsDev", lambda c: c.TieResidualStatsDev(16, 2, W, [6], H, 48, params=capi.local_warp_params(grid_y=2))),
        ("ApplyLocalWarpsDev", lambda c: c.ApplyLocalWarpsDev(D, [48, 64], W, HH, WS, [32, 32], np.zeros((2, 3, 4, 2)))),
        ("ApplyLocalWarpsDev", lambda c: c.ApplyLocalWarpsDev(D, [48], W, HH, WS, WS, np.zeros((2, 3, 4, 2)))),
        ("ApplyLocalWarpsDev", lambda c: c.ApplyLocalWarpsDev(D, D, W, HH, WS, WS, np.zeros((2, 3, 4)))),
        ("LocalRegisterDev", lambda c: c.LocalRegisterDev(16, 2, *geo)), ("LocalRegisterDev", lambda c: c.LocalRegisterDev(16, 2, *geo, grid_x=3, grid_y=2, smooth=0.5)),
        ("LocalRegisterDev", lambda c: c.LocalRegisterDev(16, 2, *geo, params=capi.local_warp_params(grid_x=0))),
        ("LocalRegisterDev", lambda c: c.LocalRegisterDev(16, 2, D, W, HH, WS, H[:1])),
        ("PairEdgesDev", lambda c: c.PairEdgesDev(16, 2, 2, 32)), ("PairEdgesDev", lambda c: c.PairEdgesDev(None, 0, 2, 0)),
        ("PairCyclesDev", lambda c: c.PairCyclesDev(np.zeros(2, capi.PAIR_EDGE), 2)), ("PairCyclesDev", lambda c: c.PairCyclesDev(np.zeros(2, capi.PAIR_EDGE), 2, cycle_tol=3.0)),
        ("PairResidualsDev", lambda c: c.PairResidualsDev(16, 2, H, None, 32)), ("PairResidualsDev", lambda c: c.PairResidualsDev(16, 2, H, [1, 1], 32)),
        ("VerifyPairsDev", lambda c: c.VerifyPairsDev(16, 2, 2, 32)), ("VerifyPairsDev", lambda c: c.VerifyPairsDev(16, 2, 2, 16, fixed=[1, 0], gate_k=2.0, bridges=0)),
        ("VerifyPairsDev", lambda c: c.VerifyPairsDev(0, 0, 0, 0, params=capi.verify_params(max_rounds=2))),
        ("GuidedSelectDev", lambda c: c.GuidedSelectDev(x["pairs"], H[1:], 16, 32, 48)),
        ("GuidedSelectDev", lambda c: c.GuidedSelectDev(x["pairs"], H[1:], 16, 32, 48, d_dist=64, radius=2.0, max_dist2=100)),
        ("GuidedSelectDev", lambda c: c.GuidedSelectDev(x["pairs"], H[1:], 16, 32, 48, params=capi.default_guided_params(ratio=0.7, reserved=1))),
        ("GuidedMatchDev", lambda c: c.GuidedMatchDev(x["pairs"], H[1:], 48)), ("GuidedMatchDev", lambda c: c.GuidedMatchDev(x["pairs"], H[1:], 48, 3.0, 7, radius=2.0)),
        ("GuidedMatchDev", lambda c: c.GuidedMatchDev(x["pairs"], H[1:], 48, params=capi.default_guided_params(ratio=0.7))),
        ("GuidedMatch", lambda c: c.GuidedMatch(x["pairs"], H[1:])), ("GuidedMatch", lambda c: c.GuidedMatch(x["pairs"], H[1:], 3.0, 7, radius=2.0)),
        ("GuidedMatch", lambda c: c.GuidedMatch(x["pairs"], H[1:], params=capi.default_guided_params(ratio=0.7))),
        ("MosaicOverviewDev", lambda c: c.MosaicOverviewDev(16, 11, 8, 36, 2, [48, 64])),
        ("MosaicOverviewDev", lambda c: c.MosaicOverviewDev(16, 11, 8, 36, 2, [48, 64], d_covers=[80, 0], d_valid_rows=96, nodata=capi.NODATA_MAP, row0=2, rows=4)),
        ("MosaicOverview", lambda c: c.MosaicOverview(np.zeros((8, 36), np.uint8), 11, 0)),
        ("MosaicOverview", lambda c: c.MosaicOverview(np.zeros((8, 36), np.uint8), 11, 0, valid=np.ones((8, 11), np.uint16), nodata=capi.NODATA_MAP, want_covers=True)),
        ("MosaicPreviewInto", lambda c: c.MosaicPreviewInto(I, None, H)),
        ("MosaicPreviewInto", lambda c: c.MosaicPreviewInto(None, [0, 1], H, geom=G, want_cover=True, render=2, level=1, nodata=1)),
        ("MosaicPreviewInto", lambda c: c.MosaicPreviewInto(I, None, H, dims=(5, 4), params=capi.preview_params(level=9))),
        ("DropFrames", lambda c: c.DropFrames()), ("DropFrames", lambda c: c.DropFrames(1)), ("FrameDev", lambda c: c.FrameDev(1)),
        ("MosaicImagesRefinedInto", lambda c: c.MosaicImagesRefinedInto(I, None, H)), ("MosaicImagesRefinedInto", lambda c: c.MosaicImagesRefinedInto(None, [0, 1], H, geom=G)),
        ("MosaicImagesRefinedInto", lambda c: c.MosaicImagesRefinedInto([I[0], None], [-1, 1], H, out=out12, pitch=40)),
        ("MosaicImagesRefinedInto", lambda c: c.MosaicImagesRefinedInto(I, None, H, out=np.zeros((2, 40), np.uint8))),
        ("MosaicImagesRefinedInto", lambda c: c.MosaicImagesRefinedInto(I, None, H, out=np.zeros((12, 40), np.uint16))),
        ("MosaicBlendedInto", lambda c: c.MosaicBlendedInto(I, None, H)),
        ("MosaicBlendedInto", lambda c: c.MosaicBlendedInto(None, [0, 1], H, keep=[1, 1], band=3, geom=G, out=np.zeros((40, 64), np.uint8), pitch=64)),
        ("close", lambda c: (c.close(), bool(c._h), c.close())),
    ]
    return calls


def module_calls(capi, x):
    """(label, callable()): every module-level wrapper of a library function, and every *_params helper with each field given"""
    H, W, HH, res = x["h9s"], x["w"], x["h"], x["res"]
    mp = np.zeros(3, capi.MATCHPAIR)
    tr = np.zeros(2, capi.IMAGE_TRANSFORM)
    h8 = np.arange(16, dtype=np.float64).reshape(2, 8)
    mom = np.zeros(2, capi.PAIR_MOMENTS)
    lw = capi.local_warp_params()
    n_stats = capi.local_warp_stats_len(2, lw.grid_x, lw.grid_y)
    return [
        ("Context", lambda: (lambda c: (c.device, bytes(c.params).hex(), c.close()))(capi.Context())),
        ("Context", lambda: (lambda c: (c.device, bytes(c.params).hex(), c.close()))(capi.Context(1, capi.default_params()))),
        ("default_params", lambda: capi.default_params()),
        ("comm_unique_id", lambda: capi.comm_unique_id()), ("comm_available", lambda: capi.comm_available()),
        ("blend_layout", lambda: capi.blend_layout(W, HH, H)), ("blend_layout", lambda: capi.blend_layout(W, HH, H, keep=[1, 0])),
        ("mosaic_layout", lambda: capi.mosaic_layout(W, HH, H)), ("resample_by_overlap", lambda: capi.resample_by_overlap(W, HH, H)),
        ("resample_by_overlap", lambda: capi.resample_by_overlap(W, HH, H, overlapT=0.5)), ("surf_pair_schedule", lambda: capi.surf_pair_schedule(4)),
        ("cover_select", lambda: capi.cover_select(W, HH, H, lambda keep: np.zeros((2, 8), np.int64))),
        ("cover_select", lambda: capi.cover_select(W, HH, H, None, order=[1, 0], pairs=x["pairs"], keep=[1, 1], step=2, max_loss=3)),
        ("cover_select", lambda: capi.cover_select(W, HH, H, None, keep=[1], params=capi.cover_params(min_depth=2))),
        ("seam_grid", lambda: capi.seam_grid(W, HH, H, 2)), ("blend_seam_grid", lambda: capi.blend_seam_grid(W, HH, H, 2)),
        ("blend_seam_grid", lambda: capi.blend_seam_grid(W, HH, H, 1, keep=[1, 1])),
        ("seam_labels_host", lambda: capi.seam_labels_host(np.zeros((1, 2), capi.SEAM_CELL))),
        ("seam_labels_host", lambda: capi.seam_labels_host(np.zeros((1, 2), capi.SEAM_CELL), seam_penalty=3)),
        ("seam_labels_host", lambda: capi.seam_labels_host(np.zeros((1, 2), capi.SEAM_CELL), params=capi.seamcut_params(ramp=2))),
        ("guided_candidates", lambda: capi.guided_candidates(8, 6, H)),
        ("guided_candidates", lambda: capi.guided_candidates(8, 6, H, have=x["pairs"], min_points=4, max_pairs=3)),
        ("guided_candidates_count", lambda: capi.guided_candidates_count(8, 6, H)),
        ("guided_candidates_count", lambda: capi.guided_candidates_count(8, 6, H, have=x["pairs"], min_points=4)),
        ("merge_pair_results", lambda: capi.merge_pair_results(res, res[:1])), ("pair_edges_host", lambda: capi.pair_edges_host(res, 2)),
        ("pair_cycles_host", lambda: capi.pair_cycles_host(np.zeros(2, capi.PAIR_EDGE), 2)),
        ("pair_cycles_host", lambda: capi.pair_cycles_host(np.zeros(2, capi.PAIR_EDGE), 2, cycle_tol=3.0)),
        ("pair_residuals_host", lambda: capi.pair_residuals_host(res, H)), ("pair_residuals_host", lambda: capi.pair_residuals_host(res, H, label=[1, 1])),
        ("verify_pairs_results", lambda: capi.verify_pairs_results(res, 2)),
        ("verify_pairs_results", lambda: capi.verify_pairs_results(res, 2, fixed=[1, 0], cycle_tol=3.0, max_rounds=2)),
        ("verify_pairs_results", lambda: capi.verify_pairs_results(res, 2, params=capi.verify_params(gate_abs=1.0))),
        ("local_warp_stats_len", lambda: capi.local_warp_stats_len(2, 4, 3)),
        ("tie_residual_stats_host", lambda: capi.tie_residual_stats_host(res, W, HH, H)),
        ("tie_residual_stats_host", lambda: capi.tie_residual_stats_host(res, W, HH, H, grid_x=3, grid_y=2)),
        ("tie_residual_stats_host", lambda: capi.tie_residual_stats_host(res, W, HH, H, params=capi.local_warp_params(grid_x=0))),
        ("tie_residual_stats_host", lambda: capi.tie_residual_stats_host(res, W, [6], H)),
        ("solve_local_warps", lambda: capi.solve_local_warps(np.zeros(n_stats, np.int64), 2)),
        ("solve_local_warps", lambda: capi.solve_local_warps(np.zeros(5, np.int64), 2, min_ties=3)),
        ("solve_local_warps", lambda: capi.solve_local_warps(np.zeros(8, np.int64), 2, params=capi.local_warp_params(grid_x=0))),
        ("undistort_fit", lambda: capi.undistort_fit(x["cam"], 8, 6)), ("undistort_fit", lambda: capi.undistort_fit(None, 8, 6)),
        ("undistort_map", lambda: capi.undistort_map(x["cam"], 8, 6)), ("undistort_map", lambda: capi.undistort_map(None, 0, 6, out_fx=90.0)),
        ("undistort_map", lambda: capi.undistort_map(x["cam"], 8, 6, params=capi.undistort_params(fill=1))),
        ("overview_layout", lambda: capi.overview_layout(11, 8, 2)), ("overview_layout", lambda: capi.overview_layout(11, 8, 0)),
        ("solve_gains", lambda: capi.solve_gains(np.zeros(1, capi.GAIN_PAIR_STATS), [4, 5])),
        ("solve_gains", lambda: capi.solve_gains(np.zeros(1, capi.GAIN_PAIR_STATS), [4, 5], sigma_g=0.2)),
        ("solve_gains", lambda: capi.solve_gains(np.zeros(1, capi.GAIN_PAIR_STATS), [4, 5], params=capi.gain_params(step=4))),
        ("solve_sharpness", lambda: capi.solve_sharpness(np.zeros(1, capi.SHARP_PAIR_STATS), 2)),
        ("solve_sharpness", lambda: capi.solve_sharpness(np.zeros(1, capi.SHARP_PAIR_STATS), 0, prior=0.1)),
        ("solve_sharpness", lambda: capi.solve_sharpness(np.zeros(1, capi.SHARP_PAIR_STATS), 2, params=capi.sharp_params(step=4))),
        ("select_sharp_frames", lambda: capi.select_sharp_frames(np.zeros(1, capi.SHARP_PAIR_STATS), 2)),
        ("select_sharp_frames", lambda: capi.select_sharp_frames(np.zeros(1, capi.SHARP_PAIR_STATS), 0, blur_ratio=0.5)),
        ("select_sharp_frames", lambda: capi.select_sharp_frames(np.zeros(1, capi.SHARP_PAIR_STATS), 2, params=capi.sharp_params(step=4))),
        ("drop_sharp_frames", lambda: capi.drop_sharp_frames(H, [1, 0])),
        ("solve_block_gains", lambda: capi.solve_block_gains(np.zeros(1, capi.BLOCK_GAIN_STATS), x["pairs"], np.zeros((2, 6), np.int64), grid_x=3, grid_y=2)),
        ("solve_block_gains", lambda: capi.solve_block_gains(np.zeros(1, capi.BLOCK_GAIN_STATS), x["pairs"], np.zeros((2, 6), np.int64))),
        ("solve_block_gains", lambda: capi.solve_block_gains(np.zeros(1, capi.BLOCK_GAIN_STATS), x["pairs"], np.zeros((2, 6), np.int64),
                                                             params=capi.block_gain_params(grid_x=0))),
        ("pair_schedule", lambda: capi.pair_schedule(4, 2)), ("pair_schedule", lambda: capi.pair_schedule(4, 2, rank=1, world=2)),
        ("write_match_pairs", lambda: capi.write_match_pairs("a.match", mp)), ("load_match_pairs", lambda: capi.load_match_pairs("a.match")),
        ("write_match_pairs_txt", lambda: capi.write_match_pairs_txt("a.txt", mp)), ("write_transforms", lambda: capi.write_transforms("t.txt", tr)),
        ("load_transforms", lambda: capi.load_transforms("t.txt")), ("load_transforms", lambda: capi.load_transforms("t.txt", tran0=True)),
        ("write_keypoints", lambda: capi.write_keypoints("k.key", np.zeros(2, capi.KEYPOINT))), ("load_keypoints", lambda: capi.load_keypoints("k.key")),
        ("write_descriptors_xml", lambda: capi.write_descriptors_xml("d.xml", np.ones((2, 4)))),
        ("write_descriptors_xml", lambda: capi.write_descriptors_xml("d.xml", np.ones(4))),
        ("load_descriptors_xml", lambda: capi.load_descriptors_xml("d.xml")),
        ("results_to_match_pairs", lambda: capi.results_to_match_pairs(res)), ("results_to_match_pairs", lambda: capi.results_to_match_pairs(res, fixed_flags=[1, 0])),
        ("global_affine_align", lambda: capi.global_affine_align(mp, 2)), ("global_affine_align", lambda: capi.global_affine_align(mp, 2, fixed=[1, 0])),
        ("select_connected_results", lambda: capi.select_connected_results(res, 2)),
        ("global_affine_align_results", lambda: capi.global_affine_align_results(res, 2)),
        ("global_affine_align_results", lambda: capi.global_affine_align_results(res, 2, fixed=[1, 0], label=[1, 1])),
        ("pair_moments_host", lambda: capi.pair_moments_host(res)),
        ("pair_normal_blocks_host", lambda: capi.pair_normal_blocks_host(res, h8, [1, 2])),
        ("global_projective_refine_results", lambda: capi.global_projective_refine_results(res, W, HH, tr)),
        ("global_projective_refine_results", lambda: capi.global_projective_refine_results(res, W, HH, tr, fixed=[1, 0], label=[1, 1],
                                                                                          params=capi.projective_params(lambda_up=5.0))),
        ("global_projective_refine", lambda: capi.global_projective_refine(mp, W, HH, tr)),
        ("global_projective_refine", lambda: capi.global_projective_refine(mp, W, HH, tr, fixed=[1, 0], params=capi.projective_params(max_iters=2))),
        ("pair_calib_blocks_host", lambda: capi.pair_calib_blocks_host(res, h8, x["cam"])),
        ("pair_calib_blocks_host", lambda: capi.pair_calib_blocks_host(res, h8, None, min_ties=4)),
        ("calibrate_lens_results", lambda: capi.calibrate_lens_results(res, x["cam"])),
        ("calibrate_lens_results", lambda: capi.calibrate_lens_results(res, None, max_iters=5, lambda_down=2.0)),
        ("calibrate_lens_results", lambda: capi.calibrate_lens_results(res, x["cam"], params=capi.calib_params(mask=7))),
        ("calibrate_lens", lambda: capi.calibrate_lens(mp, x["cam"])), ("calibrate_lens", lambda: capi.calibrate_lens(mp, x["cam"], min_ties=4)),
        ("calibrate_lens", lambda: capi.calibrate_lens(mp, x["cam"], params=capi.calib_params(mask=7))),
        ("match_pairs_to_results", lambda: capi.match_pairs_to_results(mp)),
        ("select_connected_moments", lambda: capi.select_connected_moments(mom, 2)),
        ("global_affine_align_moments", lambda: capi.global_affine_align_moments(mom, 2)),
        ("global_affine_align_moments", lambda: capi.global_affine_align_moments(mom, 2, fixed=[1, 0], label=[1, 1])),
        ("select_connected", lambda: capi.select_connected(mp, 2)),
    ] + [(name, (lambda n, k: lambda: getattr(capi, n)(**k))(name, kw)) for name, kw in sorted(PARAMS_GIVEN.items())]


# every *_params helper with each of its fields given (numbers a float32 holds exactly, integers given as floats where the field is an integer)
PARAMS_GIVEN = {
    "screen_params": dict(window=3.0, top_k=8, partners=2, min_score=5, ratio_pct=70),
    "gain_params": dict(sigma_n=5, sigma_g=0.25, channels=1.0, step=4),
    "block_gain_params": dict(sigma_n=5, sigma_g=0.25, channels=1, step=4.0, grid_x=3, grid_y=2, smooth=1),
    "sharp_params": dict(prior=1, blur_ratio=0.5, step=4.0),
    "cover_params": dict(step=4.0, min_depth=2, max_loss=1 << 40),
    "feather_params": dict(ramp=3.0), "seamline_params": dict(ramp=3.0), "median_params": dict(ramp=3, depth=4.0),
    "seamcut_params": dict(ramp=1.0, level=2, depth=3, data_weight=4, diff_weight=5, seam_penalty=6, miss_cost=7),
    "undistort_params": dict(out_fx=90, out_fy=91.5, out_cx=4, out_cy=3, fill=2.0),
    "tie_params": dict(radius=5.0, search=2, drop_mask=3, min_ncc=1),
    "local_warp_params": dict(grid_x=3.0, grid_y=2, min_ties=5, max_residual=4, max_shift=2.5, smooth=0.5, prior=1),
    "verify_params": dict(cycle_tol=3, gate_abs=1.5, gate_k=2, max_rounds=4.0, bridges=0),
    "default_guided_params": dict(radius=2, max_dist2=100.0, ratio=0.75, reserved=1),
    "preview_params": dict(render=2.0, ramp=3, level=1, nodata=1),
    "projective_params": dict(max_iters=3, prior=0.5, lambda0=0.25, lambda_up=5.0, lambda_down=2.0, min_rel_decrease=0.125),
    "calib_params": dict(max_iters=3, mask=7, min_ties=8, lambda0=0.25, lambda_up=5.0, lambda_down=2.0, min_rel_decrease=0.125),
}
# the library's own function behind each helper, and the fields whose helper default is not "the library's"
PARAMS_DEFAULT_FN = {n: "mi355_default_" + n.replace("default_", "") for n in PARAMS_GIVEN}


def _surface(capi):
    import imagemosaicing_amd as im

    def sig(f):
        try:
            return str(inspect.signature(f))
        except (TypeError, ValueError):
            return "n/a"

    def describe(mod):
        out = {}
        for n in sorted(n for n in dir(mod) if not n.startswith("_")):
            v = getattr(mod, n)
            if inspect.ismodule(v):
                continue
            out[n] = [type(v).__name__, sig(v), _crc((v.__doc__ or "").encode())] if callable(v) else [type(v).__name__, _crc(repr(v).encode())]
        return out
    methods = {n: [sig(f), _crc((f.__doc__ or "").encode())] for n, f in sorted(vars(capi.Context).items()) if callable(getattr(capi.Context, n))
               and (not n.startswith("_") or n in ("__init__", "__del__", "_chk"))}
    return {"package": {n: _crc(json.dumps(d).encode()) for n, d in describe(im).items()}, "capi": describe(capi), "Context": methods}


def _errors(capi, rec, x):
    """which wrapper raises on which return code: every module-level call under rc = 1 and rc = -2, and Context._chk"""
    out = {}
    for rc in (1, -2):
        rec.rc = rc
        for k, (name, fn) in enumerate(module_calls(capi, x)):
            r = _run(rec, name, fn)
            e = r.get("raises")
            if e is not None and e[0] == "Mi355Error":
                out["%s#%d rc=%d" % (name, k, rc)] = e[1]
        ctx = _fake_context(capi, rec)
        r = _run(rec, "synchronize", lambda: ctx.synchronize())
        out["Context._chk rc=%d" % rc] = r.get("raises", r.get("ret"))
    rec.rc = 0
    return out


def _fake_context(capi, rec):
    ctx = object.__new__(capi.Context)
    ctx.L, ctx._h, ctx.device, ctx.params = rec, C.c_void_p(1), 0, capi.default_params()
    return ctx


def record(capi, mp):
    rec = _install(capi, mp)
    x = _inputs(capi)
    ctx = _fake_context(capi, rec)
    calls = context_calls(capi, x)
    public = {n for n, f in vars(capi.Context).items() if callable(getattr(capi.Context, n)) and not n.startswith("_")}
    driven = {n for n, _ in calls}
    assert len(SKIP) <= 3 and driven | set(SKIP) == public and not driven & set(SKIP), sorted(public ^ (driven | set(SKIP)))
    out = {"surface": _surface(capi),
           "context": [_run(rec, name, (lambda f: lambda: f(ctx))(fn)) for name, fn in calls],
           "module": [_run(rec, name, fn) for name, fn in module_calls(capi, x)]}
    out["errors"] = _errors(capi, rec, x)
    return json.loads(json.dumps(out))


def test_calls_and_surface_equal_the_recorded_ones(capi, monkeypatch):
    got = record(capi, monkeypatch)
    want = json.load(open(GOLDEN))
    assert sorted(got) == sorted(want)
    assert got["surface"] == want["surface"]
    for part in ("context", "module"):
        assert len(got[part]) == len(want[part])
        for g, w in zip(got[part], want[part]):
            assert g == w, (part, w["call"])
    assert got["errors"] == want["errors"]


@pytest.mark.parametrize("helper", ["projective_params", "calib_params"])
def test_unknown_params_keyword_is_a_type_error(capi, helper):
    with pytest.raises(TypeError):
        getattr(capi, helper)(max_iter=3)                     # a misspelt max_iters used to be set on the Python object and ignored
    assert getattr(capi, helper)(max_iters=3).max_iters == 3


@pytest.mark.parametrize("helper", sorted(PARAMS_GIVEN))
def test_params_helper_without_arguments_gives_the_librarys_defaults(capi, helper):
    p = getattr(capi, helper)()
    q = type(p)()
    getattr(capi.load_library(), PARAMS_DEFAULT_FN[helper])(C.byref(q))
    assert bytes(p) == bytes(q)


if __name__ == "__main__":
    from imagemosaicing_amd import capi as _capi
    with pytest.MonkeyPatch.context() as _mp:
        _g = record(_capi, _mp)
    with open(GOLDEN, "w") as _f:
        _f.write("{\n")
        _f.write('"surface": ' + json.dumps(_g["surface"], sort_keys=True, separators=(",", ":")) + ",\n")
        for _part in ("context", "module"):
            _f.write('"%s": [\n' % _part + ",\n".join(json.dumps(c, sort_keys=True, separators=(",", ":")) for c in _g[_part]) + "\n],\n")
        _f.write('"errors": ' + json.dumps(_g["errors"], sort_keys=True, indent=0) + "\n}\n")
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
