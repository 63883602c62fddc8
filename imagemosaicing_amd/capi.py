"""ctypes binding of libmi355mosaic.so (include/mi355_mosaic.h).  No torch types cross this boundary:
device buffers are passed as integer addresses (e.g. tensor.data_ptr())."""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

SFPOINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("id", "<i4")])
KEYPOINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                     ("octave", "<i4"), ("class_id", "<i4")])
DMATCH = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])
MATCHPAIR = np.dtype([("ax", "<f4"), ("ay", "<f4"), ("aid", "<i4"), ("ai", "<i4"), ("af", "<i4"),
                      ("bx", "<f4"), ("by", "<f4"), ("bid", "<i4"), ("bi", "<i4"), ("bf", "<i4")])
PAIR_RESULT = np.dtype([("i", "<i4"), ("j", "<i4"), ("n_in", "<i4"), ("n_selected", "<i4"), ("ok", "<i4"),
                        ("accepted", "<i4"), ("H", "<f4", (9,)), ("_pad", "<i4"),
                        ("a", SFPOINT, (400,)), ("b", SFPOINT, (400,))])
CHIPINFO = np.dtype([("x0", "<i4"), ("y0", "<i4"), ("w", "<i4"), ("h", "<i4"), ("img", "<i4"),
                     ("sx", "<f4"), ("sy", "<f4"), ("quad", "<f4", (8,))])
IMAGE_TRANSFORM = np.dtype([("m", "<f4", (9,)), ("fixed", "<i4")])
PAIR_MOMENTS = np.dtype([("i", "<i4"), ("j", "<i4"), ("n_in", "<i4"), ("_pad", "<i4"), ("aa", "<f8", (6,)), ("ab", "<f8", (9,)), ("bb", "<f8", (6,))])
FEATURE_HEADER = np.dtype([("img_id", "<i4"), ("n_kp", "<i4"), ("w", "<i4"), ("h", "<i4")])
FEATURE_RECORD_BYTES = 319488
# one chunk record of a frame's rows [row0, row0 + rows) (mi355_feature_chunk_header): a frame of n_kp keypoints takes max(1, ceil(n_kp / 2048))
FEATURE_CHUNK_HEADER = np.dtype([("img_id", "<i4"), ("n_kp", "<i4"), ("w", "<i4"), ("h", "<i4"), ("chunk", "<i4"), ("n_chunks", "<i4"),
                                 ("row0", "<i4"), ("rows", "<i4")])
FEATURE_CHUNK_ROWS = 2048
assert FEATURE_CHUNK_HEADER.itemsize == 32
assert SFPOINT.itemsize == 12 and KEYPOINT.itemsize == 28 and MATCHPAIR.itemsize == 40 and PAIR_RESULT.itemsize == 9664 and PAIR_MOMENTS.itemsize == 184


class Params(C.Structure):
    _fields_ = [("nfeatures", C.c_int32), ("n_octave_layers", C.c_int32), ("contrast_threshold", C.c_float),
                ("edge_threshold", C.c_float), ("sigma", C.c_float), ("max_selected", C.c_int32),
                ("select_fraction", C.c_double), ("grid_x", C.c_int32), ("grid_y", C.c_int32), ("min_inliers", C.c_int32),
                ("ransac_dist", C.c_float), ("sample_times", C.c_int32), ("pair_window", C.c_int32), ("ratio", C.c_float)]


class ScreenParams(C.Structure):
    _fields_ = [("top_k", C.c_int32), ("partners", C.c_int32), ("min_score", C.c_int32), ("ratio_pct", C.c_int32), ("window", C.c_int32)]


class GainParams(C.Structure):
    _fields_ = [("sigma_n", C.c_float), ("sigma_g", C.c_float), ("channels", C.c_int32), ("step", C.c_int32)]


class BlockGainParams(C.Structure):
    _fields_ = [("sigma_n", C.c_float), ("sigma_g", C.c_float), ("channels", C.c_int32), ("step", C.c_int32), ("grid_x", C.c_int32),
                ("grid_y", C.c_int32), ("smooth", C.c_int32), ("reserved", C.c_int32)]


class SharpParams(C.Structure):
    _fields_ = [("prior", C.c_float), ("blur_ratio", C.c_float), ("step", C.c_int32), ("reserved", C.c_int32)]


class CoverParams(C.Structure):
    _fields_ = [("step", C.c_int32), ("min_depth", C.c_int32), ("max_loss", C.c_int64)]


class FeatherParams(C.Structure):
    _fields_ = [("ramp", C.c_int32), ("reserved", C.c_int32 * 3)]


class SeamlineParams(C.Structure):
    _fields_ = [("ramp", C.c_int32), ("reserved", C.c_int32 * 3)]


class MedianParams(C.Structure):
    _fields_ = [("ramp", C.c_int32), ("depth", C.c_int32), ("reserved", C.c_int32 * 2)]


class SeamCutParams(C.Structure):
    _fields_ = [("ramp", C.c_int32), ("level", C.c_int32), ("depth", C.c_int32), ("data_weight", C.c_int32), ("diff_weight", C.c_int32),
                ("seam_penalty", C.c_int32), ("miss_cost", C.c_int32), ("reserved", C.c_int32)]


class SeamReport(C.Structure):
    _fields_ = [("energy_before", C.c_int64), ("energy_after", C.c_int64), ("changed", C.c_int32), ("fallback", C.c_int32)]


SEAM_CELL = np.dtype([("frame", "<u2", 8), ("omega", "u1", 8), ("gray", "u1", 8)])     # mi355_seam_cell, 32 bytes


class Camera(C.Structure):
    """mi355_camera: a Brown-Conrady camera in pixels, OpenCV's coefficient order and signs"""
    _fields_ = [(n, C.c_double) for n in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")]


class UndistortParams(C.Structure):
    _fields_ = [("out_fx", C.c_double), ("out_fy", C.c_double), ("out_cx", C.c_double), ("out_cy", C.c_double), ("fill", C.c_int32),
                ("reserved", C.c_int32 * 3)]


class PreviewParams(C.Structure):
    _fields_ = [("render", C.c_int32), ("ramp", C.c_int32), ("level", C.c_int32), ("nodata", C.c_int32), ("reserved", C.c_int32 * 4)]


class LocalWarpParams(C.Structure):
    _fields_ = [("grid_x", C.c_int32), ("grid_y", C.c_int32), ("min_ties", C.c_int32), ("reserved", C.c_int32), ("max_residual", C.c_double),
                ("max_shift", C.c_double), ("smooth", C.c_double), ("prior", C.c_double)]


# mi355_local_warp_report: what the local registration's solve says of one frame
LOCAL_WARP_REPORT = np.dtype([("n_ties", "<i8"), ("rej_den", "<i8"), ("rej_residual", "<i8"), ("rej_side", "<i8"), ("rms_before", "<f8"),
                              ("rms_after", "<f8"), ("max_shift", "<f8"), ("solved", "<i4"), ("_pad", "<i4")])
assert C.sizeof(LocalWarpParams) == 48 and LOCAL_WARP_REPORT.itemsize == 64

NODATA_NONE, NODATA_ZERO, NODATA_MAP = 0, 1, 2


# mi355_gain_pair_stats: the overlap statistics of one listed pair (positions a, b in the frame list)
GAIN_PAIR_STATS = np.dtype([("a", "<i4"), ("b", "<i4"), ("n", "<i8"), ("sum_a", "<i8", (3,)), ("sum_b", "<i8", (3,))])
assert GAIN_PAIR_STATS.itemsize == 64
# mi355_block_gain_stats: the statistics of one (cell_a, cell_b) of listed pair `pair` (an index into the pair list)
BLOCK_GAIN_STATS = np.dtype([("pair", "<i4"), ("cell_a", "<i4"), ("cell_b", "<i4"), ("reserved", "<i4"), ("n", "<i8"), ("sum_a", "<i8", (3,)),
                             ("sum_b", "<i8", (3,))])
# mi355_sharp_pair_stats / mi355_sharp_frame_stats: Laplacian energy and centre gray of one listed pair / one frame ("frame sharpness")
SHARP_PAIR_STATS = np.dtype([("a", "<i4"), ("b", "<i4"), ("n", "<i8"), ("e_a", "<i8"), ("e_b", "<i8"), ("s_a", "<i8"), ("s_b", "<i8")])
SHARP_FRAME_STATS = np.dtype([("n", "<i8"), ("e", "<i8"), ("s", "<i8")])
SHARP_KEPT, SHARP_DROPPED, SHARP_CUT_VERTEX, SHARP_NO_PAIR = 0, 1, 2, 3
assert SHARP_PAIR_STATS.itemsize == 48 and SHARP_FRAME_STATS.itemsize == 24 and C.sizeof(SharpParams) == 16
# mi355_cover_frame_stats: the lattice points a frame covers by their depth ("cover depth"); the selection's status codes
COVER_FRAME_STATS = np.dtype([("at_depth", "<i8", (8,))])
COVER_BINS = 9
COVER_NOT_CANDIDATE, COVER_DROPPED, COVER_KEPT_COVERAGE, COVER_CUT_VERTEX, COVER_NOT_EXAMINED = 0, 1, 2, 3, 4
COVER_STATS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p)      # mi355_cover_stats_fn(user, keep, frame_stats)
assert COVER_FRAME_STATS.itemsize == 64 and C.sizeof(CoverParams) == 16
PAIR_NORMAL_BLOCK = np.dtype([("i", "<i4"), ("j", "<i4"), ("n_in", "<i4"), ("_pad", "<i4"), ("cost", "<f8"), ("g", "<f8", (16,)), ("N", "<f8", (136,))])


class ProjectiveParams(C.Structure):
    _fields_ = [("max_iters", C.c_int32), ("reserved", C.c_int32), ("prior", C.c_double), ("lambda0", C.c_double), ("lambda_up", C.c_double),
                ("lambda_down", C.c_double), ("min_rel_decrease", C.c_double)]


class ProjectiveReport(C.Structure):
    _fields_ = [("trials", C.c_int32), ("accepted", C.c_int32), ("n_free", C.c_int32), ("n_pairs_used", C.c_int32), ("n_points", C.c_int64),
                ("cost0", C.c_double), ("cost_data", C.c_double), ("cost_prior", C.c_double), ("lambda_", C.c_double)]

    def as_dict(self):
        return {n.rstrip("_"): getattr(self, n) for n, _ in self._fields_}


# mi355_pair_calib_block: the normal-equation block of one pair record for the lens self-calibration (8 state values | k1 k2 p1 p2 k3)
PAIR_CALIB_BLOCK = np.dtype([("i", "<i4"), ("j", "<i4"), ("n_in", "<i4"), ("n_bad", "<i4"), ("cost", "<f8"), ("g", "<f8", (13,)), ("N", "<f8", (91,))])
CALIB_K1, CALIB_K2, CALIB_P1, CALIB_P2, CALIB_K3 = 1, 2, 4, 8, 16


class CalibParams(C.Structure):
    _fields_ = [("max_iters", C.c_int32), ("mask", C.c_int32), ("min_ties", C.c_int32), ("reserved", C.c_int32), ("lambda0", C.c_double),
                ("lambda_up", C.c_double), ("lambda_down", C.c_double), ("min_rel_decrease", C.c_double)]


class CalibReport(C.Structure):
    _fields_ = [("trials", C.c_int32), ("accepted", C.c_int32), ("n_pairs_used", C.c_int32), ("n_unused_records", C.c_int32), ("n_points", C.c_int64),
                ("cost0", C.c_double), ("cost", C.c_double), ("lambda_", C.c_double)]

    def as_dict(self):
        return {n.rstrip("_"): getattr(self, n) for n, _ in self._fields_}


assert PAIR_CALIB_BLOCK.itemsize == 856 and C.sizeof(CalibParams) == 48 and C.sizeof(CalibReport) == 48


class TieParams(C.Structure):
    _fields_ = [("radius", C.c_int32), ("search", C.c_int32), ("drop_mask", C.c_int32), ("reserved", C.c_int32), ("min_ncc", C.c_float)]


# mi355_tie_report: what the tie refinement says of one pair record
TIE_REPORT = np.dtype([("i", "<i4"), ("j", "<i4"), ("n_in", "<i4"), ("n_out", "<i4"), ("flags", "<i4"), ("count", "<i4", (8,)), ("_pad", "<i4"),
                       ("ncc_q_sum", "<i8")])
TIE_NONE, TIE_REFINED, TIE_EDGE, TIE_FLAT, TIE_LOW, TIE_BORDER = 0, 1, 2, 3, 4, 5
TIE_FLAG_NOT_ACCEPTED, TIE_FLAG_NO_FRAME, TIE_FLAG_BAD_RECORD, TIE_FLAG_DEMOTED = 1, 2, 4, 8
assert TIE_REPORT.itemsize == 64 and C.sizeof(TieParams) == 20
assert PAIR_NORMAL_BLOCK.itemsize == 1240 and C.sizeof(ProjectiveParams) == 48 and C.sizeof(ProjectiveReport) == 56
assert BLOCK_GAIN_STATS.itemsize == 72 and C.sizeof(BlockGainParams) == 32
assert C.sizeof(Camera) == 72 and C.sizeof(UndistortParams) == 48


# ---- pair verification (mi355_pair_edges_*, mi355_pair_cycles_*, mi355_pair_residuals_*, mi355_verify_pairs_*; csrc/verify.hip) ----
class VerifyParams(C.Structure):
    _fields_ = [("cycle_tol", C.c_double), ("gate_abs", C.c_double), ("gate_k", C.c_double), ("max_rounds", C.c_int32), ("bridges", C.c_int32)]


PAIR_EDGE = np.dtype([("i", "<i4"), ("j", "<i4"), ("n_in", "<i4"), ("flags", "<i4"), ("box", "<f4", (4,)), ("F", "<f8", (9,)), ("B", "<f8", (9,))])
PAIR_CYCLE = np.dtype([("n_ok", "<i4"), ("n_bad", "<i4"), ("min_e2", "<f8")])
PAIR_RESIDUAL = np.dtype([("i", "<i4"), ("j", "<i4"), ("n_used", "<i4"), ("n_den", "<i4"), ("sum_r2", "<f8"), ("max_r2", "<f8")])
VERIFY_REPORT = np.dtype([("i", "<i4"), ("j", "<i4"), ("n_in", "<i4"), ("verdict", "<i4"), ("n_ok", "<i4"), ("n_bad", "<i4"), ("round", "<i4"),
                          ("flags", "<i4"), ("min_e2", "<f8"), ("rms", "<f8"), ("max_r2", "<f8"), ("reserved", "<f8")])
VERIFY_SUMMARY = np.dtype([("count", "<i4", (8,)), ("rounds", "<i4"), ("n_labelled", "<i4"), ("reserved", "<i4", (2,)), ("s", "<f8"), ("gate", "<f8")])
EDGE_USABLE, EDGE_TESTABLE = 1, 2
VERDICT_NOT_USED, VERDICT_VERIFIED, VERDICT_ADMITTED, VERDICT_BRIDGE, VERDICT_REJECTED, VERDICT_UNDECIDED = 0, 1, 2, 3, 4, 5
VERIFY_SUSPECT = 1
assert PAIR_EDGE.itemsize == 176 and PAIR_CYCLE.itemsize == 16 and PAIR_RESIDUAL.itemsize == 32
assert C.sizeof(VerifyParams) == 32 and VERIFY_REPORT.itemsize == 64 and VERIFY_SUMMARY.itemsize == 64


# ---- guided matching (mi355_guided_select_dev, mi355_guided_match*, mi355_guided_candidates, mi355_merge_pair_results; csrc/guided.hip) ----
class GuidedParams(C.Structure):
    _fields_ = [("radius", C.c_float), ("max_dist2", C.c_int32), ("ratio", C.c_float), ("reserved", C.c_int32)]


assert C.sizeof(GuidedParams) == 16


class Mi355Error(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("mi355 error %d: %s" % (code, msg))
        self.code = code


def lib_path():
    # MI355_LIB: a kernel A/B build of the same library (scratch/build_variant.sh); measurement only
    return os.environ.get("MI355_LIB") or os.path.join(_HERE, "libmi355mosaic.so")


def load_library():
    """Loads the in-tree HIP library.  Fails loudly when it has not been built (python -m imagemosaicing_amd.build)."""
    global _LIB
    if _LIB is None:
        p = lib_path()
        if not os.path.exists(p):
            raise ImportError("libmi355mosaic.so is not built: run `python -m imagemosaicing_amd.build` "
                              "(there is no CPU fallback for the HIP path)")
        # One HIP runtime per process: PyTorch-ROCm wheels bundle their own libamdhip64.so.7 / libhsa-runtime64.
        # When torch is present (bench.py, tests: device memory + torch.distributed), import it FIRST so that this
        # library's DT_NEEDED libamdhip64.so.7 resolves to the runtime torch already loaded instead of a second copy
        # from /opt/rocm (two runtimes in one process cannot both own the GPU).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(p)
        L.mi355_last_error.restype = C.c_char_p
        L.mi355_last_error.argtypes = [C.c_void_p]
        L.mi355_create.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_int]
        L.mi355_destroy.argtypes = [C.c_void_p]
        L.mi355_free.argtypes = [C.c_void_p]
        _LIB = L
    return _LIB


def default_params():
    p = Params()
    load_library().mi355_default_params(C.byref(p))
    return p


# ---- marshalling: one implementation of each job the wrappers below share ------------------------------------------------
def _params(cls, default_fn_name, fields):
    """cls as the library's default_fn_name fills it, then the given fields (None: not given) assigned, each coerced by its declared ctypes
    type.  A name that is not a field is a TypeError."""
    p = cls()
    getattr(load_library(), default_fn_name)(C.byref(p))
    kinds = dict(cls._fields_)
    for name, v in fields.items():
        if name not in kinds:
            raise TypeError("%s has no field %r" % (cls.__name__, name))
        if v is not None:
            setattr(p, name, float(v) if kinds[name] in (C.c_float, C.c_double) else int(v))
    return p


def _resolve(params, maker, kw):
    """the params object a wrapper was given, or maker's from the keyword fields"""
    return params if params is not None else maker(**kw)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _ref(x):
    """a structure by reference; None stays None (the library's NULL)"""
    return C.byref(x) if x is not None else None


def _arr(a, dtype):
    """a as a contiguous array of dtype; None stays None (the library's NULL)"""
    return None if a is None else np.ascontiguousarray(a, dtype)


def _dptr(x):
    """a device address (0 / None: NULL) as the pointer argument of a call"""
    return C.c_void_p(int(x or 0) or None)


def _dptrs(xs, at_least=0):
    """device addresses (0 / None: NULL) as an array of pointers; None: no array"""
    if xs is None:
        return None
    return (C.c_void_p * max(len(xs), at_least))(*[int(x or 0) or None for x in xs])


def _dev_frames(d_imgs, w, h, ws, h9s=None):
    """n, pointers, w, h, ws, h9s of a list of device frames as every call takes them.  d_imgs None: no pointers (a call that reads no
    pixels), ws None: no pitches, h9s None: the call takes no transforms."""
    w, h = np.ascontiguousarray(w, np.int32), np.ascontiguousarray(h, np.int32)
    n = len(w)
    return n, _dptrs(d_imgs, n), w, h, _arr(ws, np.int32), _arr(h9s, np.float32)


def _host_frames(imgs):
    """n, the images as contiguous uint8 arrays, their pointers, w, h, ws.  The pointer array holds addresses only: the caller keeps the
    returned images referenced until its call has returned."""
    imgs = [np.ascontiguousarray(i, np.uint8) for i in imgs]
    ptrs = (C.c_void_p * len(imgs))(*[i.ctypes.data for i in imgs])
    w = np.array([i.shape[1] for i in imgs], np.int32)
    h = np.array([i.shape[0] for i in imgs], np.int32)
    ws = np.array([i.strides[0] for i in imgs], np.int32)
    return len(imgs), imgs, ptrs, w, h, ws


def _geom(w, h, h9s):
    """n, w, h, h9s of a survey given by its frames' sizes and transforms alone"""
    return len(w), np.ascontiguousarray(w, np.int32), np.ascontiguousarray(h, np.int32), np.ascontiguousarray(h9s, np.float32)


def _h9rows(h9s):
    """the transforms as float32 rows of 9, whichever shape they come in"""
    return np.ascontiguousarray(h9s, np.float32).reshape(-1, 9)


def _img_geom(img):
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape[:2]
    ch = img.shape[2] if img.ndim == 3 else 1
    return img, w, h, img.strides[0], ch


def _owned(L, ptr, count, dtype, copy=True, free=True, want=True):
    """count items of dtype from a library-owned host buffer: a private copy, or (copy=False) a view valid as long as the library says.
    free: the buffer goes back through mi355_free afterwards; want=False: it only goes back, nothing is copied."""
    out = None
    if want:
        if not ptr or count == 0:
            out = np.zeros(0, dtype)
        else:
            raw = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(count * np.dtype(dtype).itemsize,))
            out = (raw.copy() if copy else raw).view(dtype)
    if free:
        L.mi355_free(ptr)
    return out


def _host_chk(rc, what=None, positive=True):
    """the error path of the wrappers that take no ctx: raises Mi355Error with the fixed text `what`, or (None) the library's last error.
    positive: rc > 0 is a failure too."""
    if rc < 0 or (positive and rc != 0):
        raise Mi355Error(rc, what if what is not None else (load_library().mi355_last_error(None) or b"").decode())
    return rc


def _load(fn_name, what, dtype, *args):
    """the load_* shape: fn(args..., &array, &count) hands back a malloc'd array of dtype, which is copied and freed"""
    L = load_library()
    ptr, n = C.c_void_p(), C.c_int(0)
    _host_chk(getattr(L, fn_name)(*args, C.byref(ptr), C.byref(n)), what)
    return _owned(L, ptr, n.value, dtype)


def _write(fn_name, what, path, a, *dims):
    """the write_* shape: fn(path, array, its dims...)"""
    L = load_library()
    _host_chk(getattr(L, fn_name)(path.encode(), _p(a), *dims), what)


class Context:
    """One GPU context (mi355_create).  Methods are named after the reference functions they replace."""

    def __init__(self, device=0, params=None):
        self.L = load_library()
        self._h = C.c_void_p()
        _host_chk(self.L.mi355_create(C.byref(self._h), _ref(params), int(device)))
        self.params = _resolve(params, default_params, {})
        self.device = int(device)

    def close(self):
        if self._h:
            self.L.mi355_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc < 0:
            raise Mi355Error(rc, (self.L.mi355_last_error(self._h) or b"").decode())
        return rc

    # ---- the forms every render comes in.  `lead` holds the family's own arguments, which stand between the transforms and the outputs ----
    def _render_host(self, fn, imgs, h9s, lead=(), want_pixels=True, extra=None):
        """host images in, the library's canvas out: fn(ctx, frames, n, h9s, *lead, &canvas, &cw, &ch, &cws[, &map]).  extra: None where fn has no
        map output, else (wanted, dtype) of the [ch, cw] map behind the canvas.  Returns (canvas rows x cws or None, cw, ch, cws[, map])."""
        n, imgs, ptrs, w, h, ws = _host_frames(imgs)
        h9s = _arr(h9s, np.float32)
        canvas, more = C.c_void_p(), C.c_void_p()
        cw, ch, cws = C.c_int(), C.c_int(), C.c_int()
        tail = () if extra is None else (C.byref(more) if extra[0] else None,)
        self._chk(fn(self._h, ptrs, _p(w), _p(h), _p(ws), n, _p(h9s), *lead, C.byref(canvas), C.byref(cw), C.byref(ch), C.byref(cws), *tail))
        buf = _owned(self.L, canvas, ch.value * cws.value, np.uint8, want=want_pixels)
        out = (buf.reshape(ch.value, cws.value) if want_pixels else None, cw.value, ch.value, cws.value)
        if extra is None or not extra[0]:
            return out
        return out + (_owned(self.L, more, ch.value * cw.value, extra[1]).reshape(ch.value, cw.value),)

    def _render_dev(self, fn, d_imgs, w, h, ws, h9s, lead, d_canvas, cw, ch, cws, maps=(), stripe=None):
        """device frames into a device canvas: fn(ctx, frames, n, h9s, *lead, canvas, cw, ch, cws, *maps[, row0, rows]).  maps: the device
        addresses of the render's per-pixel maps; stripe: (row0, rows), rows < 0 = the whole canvas, None where fn takes no stripe."""
        n, ptrs, w, h, ws, h9s = _dev_frames(d_imgs, w, h, ws, h9s)
        rows = () if stripe is None else (int(stripe[0]), int(stripe[1] if stripe[1] >= 0 else ch))
        self._chk(fn(self._h, ptrs, _p(w), _p(h), _p(ws), n, _p(h9s), *lead, _dptr(d_canvas), int(cw), int(ch), int(cws),
                     *[_dptr(m) for m in maps], *rows))

    def _render_into(self, fn, imgs, img_ids, h9s, lead, layout, out, pitch, geom):
        """kept frames and / or host images into caller memory: fn(ctx, sources, n, h9s, *lead, out, pitch, cw, ch), the canvas's (cw, ch)
        being the first two of layout(w, h, h9s).  Returns (out, cw, ch)."""
        ptrs, ids, w, h, ws, _keep = self._into_args(imgs, img_ids, geom)
        h9s = _arr(h9s, np.float32)
        cw, ch = layout(w, h, h9s)[:2]
        out, pitch = self._out_array(out, pitch, cw, ch)
        self._chk(fn(self._h, ptrs, _p(ids), _p(w), _p(h), _p(ws), len(ids), _p(h9s), *lead, C.c_void_p(out.ctypes.data), int(pitch),
                     int(cw), int(ch)))
        return out, cw, ch

    def _render_cover(self, fn, w, h, h9s, lead, row0, rows, first=()):
        """which frames a stripe of a render reads, from the geometry alone: fn(ctx, *first, w, h, n, h9s, *lead, row0, rows, need)"""
        n, w, h, h9s = _geom(w, h, h9s)
        need = np.zeros(n, np.uint8)
        self._chk(fn(self._h, *first, _p(w), _p(h), n, _p(h9s), *lead, int(row0), int(rows), _p(need)))
        return need

    def _chips(self, fn, *args):
        """fn(ctx, *args, &n, &chips, &imgs, &masks, &cw, &ch): the library-owned chips of a warp stage as ChipsAndMasks' dictionary"""
        nch = C.c_int(0)
        chips = C.c_void_p()
        cimgs = C.POINTER(C.c_void_p)()
        masks = C.POINTER(C.c_void_p)()
        cw, ch = C.c_int(), C.c_int()
        self._chk(fn(self._h, *args, C.byref(nch), C.byref(chips), C.byref(cimgs), C.byref(masks), C.byref(cw), C.byref(ch)))
        nv = nch.value
        info = _owned(self.L, chips, nv, CHIPINFO)
        out_c, out_m = [], []
        for v in range(nv):
            cwv, chv = int(info[v]["w"]), int(info[v]["h"])
            cws_, mws = (cwv * 3 + 3) & ~3, (cwv + 3) & ~3
            out_c.append(_owned(self.L, C.c_void_p(cimgs[v]), chv * cws_, np.uint8).reshape(chv, cws_))
            out_m.append(_owned(self.L, C.c_void_p(masks[v]), chv * mws, np.uint8).reshape(chv, mws))
        self.L.mi355_free(C.cast(cimgs, C.c_void_p))
        self.L.mi355_free(C.cast(masks, C.c_void_p))
        return dict(cw=cw.value, ch=ch.value, chips=info, chip_imgs=out_c, masks=out_m)

    # ---- plumbing ----------------------------------------------------------------------------
    def set_stream(self, hip_stream):
        self._chk(self.L.mi355_set_stream(self._h, C.c_void_p(hip_stream or 0)))

    def synchronize(self):
        self._chk(self.L.mi355_synchronize(self._h))

    def set_option(self, name, value):
        self._chk(self.L.mi355_set_option(self._h, name.encode(), int(value)))
        if name == "nfeatures":
            self.params.nfeatures = int(value)

    def profile_enable(self, on=True):
        self._chk(self.L.mi355_profile_enable(self._h, int(bool(on))))

    def profile_only(self, cls=None):
        self._chk(self.L.mi355_profile_only(self._h, (cls or "").encode()))

    def profile_reset(self):
        self._chk(self.L.mi355_profile_reset(self._h))

    def profile_get(self, cls):
        ms, n, b = C.c_double(), C.c_int64(), C.c_double()
        self._chk(self.L.mi355_profile_get(self._h, cls.encode(), C.byref(ms), C.byref(n), C.byref(b)))
        return ms.value, n.value, b.value

    # ---- features (SiftExtraction_Thread, MosaicWithoutPos.cpp:4832-4887) ------------------------
    def SiftExtract(self, img_id, bgr, max_kp=None):
        img, w, h, ws, ch = _img_geom(bgr)
        assert ch == 3
        max_kp = max_kp or max(int(self.params.nfeatures), 2048)      # nfeatures + ties with the last one (retainBest), up to the record's 2048
        kp = np.zeros(max_kp, KEYPOINT)
        desc = np.zeros((max_kp, 128), np.float32)
        n = C.c_int(0)
        self._chk(self.L.mi355_sift_extract(self._h, int(img_id), _p(img), w, h, ws, _p(kp), _p(desc), max_kp, C.byref(n)))
        k = min(n.value, max_kp)
        return kp[:k].copy(), desc[:k].copy()

    def SiftExtractHost(self, img_id, bgr):
        """Host frame in, nothing back: the frame is copied into the library's staging ring and joins a batch like a device
        frame (mi355_sift_extract with kp = desc = n_kp = NULL).  The array may be reused as soon as the call returns."""
        img, w, h, ws, ch = _img_geom(bgr)
        assert ch == 3
        self._chk(self.L.mi355_sift_extract(self._h, int(img_id), _p(img), w, h, ws, None, None, 0, None))

    def SiftExtractDev(self, img_id, d_bgr, w, h, ws, want_count=False):
        """Asynchronous unless want_count: the frame is enqueued on one of the library's SIFT streams and the call
        returns; the keypoint count is adopted at the next MatchPairs / GetFeatures / synchronize."""
        if not want_count:
            self._chk(self.L.mi355_sift_extract_dev(self._h, int(img_id), C.c_void_p(int(d_bgr)), int(w), int(h), int(ws), None))
            return None
        n = C.c_int(0)
        self._chk(self.L.mi355_sift_extract_dev(self._h, int(img_id), C.c_void_p(int(d_bgr)), int(w), int(h), int(ws), C.byref(n)))
        return n.value

    def GetFeatures(self, img_id, max_kp=4096):
        kp = np.zeros(max_kp, KEYPOINT)
        desc = np.zeros((max_kp, 128), np.float32)
        n = C.c_int(0)
        self._chk(self.L.mi355_get_features(self._h, int(img_id), _p(kp), _p(desc), max_kp, C.byref(n)))
        return kp[:n.value].copy(), desc[:n.value].copy()

    def SetFeatures(self, img_id, kp, desc, w, h):
        kp = np.ascontiguousarray(kp, KEYPOINT)
        desc = np.ascontiguousarray(desc, np.float32)
        self._chk(self.L.mi355_set_features(self._h, int(img_id), _p(kp), _p(desc), len(kp), int(w), int(h)))

    def DropFeatures(self, img_id=-1):
        self._chk(self.L.mi355_drop_features(self._h, int(img_id)))

    # ---- match (GetMatchedPairsOneToAllSIFTThread j-loop, MosaicWithoutPos.cpp:5084-5232) ----------
    def MatchPairs(self, pairs, ransac_dist=2.5, seed=1):
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        out = np.zeros(len(pairs), PAIR_RESULT)
        self._chk(self.L.mi355_match_pairs(self._h, _p(pairs), len(pairs), C.c_float(ransac_dist), C.c_uint32(seed), _p(out)))
        return out

    def MatchPairsDev(self, pairs, d_out, ransac_dist=2.5, seed=1):
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        self._chk(self.L.mi355_match_pairs_dev(self._h, _p(pairs), len(pairs), C.c_float(ransac_dist), C.c_uint32(seed), C.c_void_p(int(d_out))))

    # ---- descriptor-screened pair schedule (mi355_screen_pairs, csrc/screen.hip) ----------------------------------
    def ScreenPairs(self, img_ids, window=0, top_k=256, partners=None, min_score=None, ratio_pct=80, rank=0, world=1, return_scores=False):
        """the screened schedule over img_ids: [n_pairs, 2] image ids (positions a < b, sorted by (a, b), a mod world == rank); with
        return_scores also the pairs' scores.  partners / min_score default to the library's (screen_params())."""
        ids = np.ascontiguousarray(img_ids, np.int32).reshape(-1)
        p = screen_params(window=window, top_k=top_k, partners=partners, min_score=min_score, ratio_pct=ratio_pct)
        cap = len(ids) * p.partners if p.partners > 0 else 0
        n = C.c_int(0)
        while True:
            out = np.zeros((max(cap, 1), 2), np.int32)
            sc = np.zeros(max(cap, 1), np.int32)
            rc = self.L.mi355_screen_pairs(self._h, _p(ids), len(ids), C.byref(p), int(rank), int(world), _p(out), _p(sc), cap, C.byref(n))
            if rc == -1 and n.value > cap:
                cap = n.value
                continue
            self._chk(rc)
            break
        pairs = out[:n.value].copy()
        return (pairs, sc[:n.value].copy()) if return_scores else pairs

    def ScreenScoresDev(self, img_ids, d_scores, **params):
        """the n x n int32 score matrix of img_ids into device memory d_scores (-1 on the diagonal and outside the window)"""
        ids = np.ascontiguousarray(img_ids, np.int32).reshape(-1)
        p = screen_params(**params)
        self._chk(self.L.mi355_screen_scores_dev(self._h, _p(ids), len(ids), C.byref(p), C.c_void_p(int(d_scores))))

    def BFMatch(self, img_i, img_j, sorted_=True, max_matches=2048):
        m = np.zeros(max_matches, DMATCH)
        d2 = np.zeros(max_matches, np.int32)
        s2 = np.zeros(max_matches, np.int32)
        n = C.c_int(0)
        self._chk(self.L.mi355_bf_match(self._h, int(img_i), int(img_j), int(bool(sorted_)), _p(m), _p(d2), _p(s2), max_matches, C.byref(n)))
        k = min(n.value, max_matches)
        return m[:k].copy(), d2[:k].copy(), s2[:k].copy()

    # ---- stand-alone reference functions ------------------------------------------------------------
    def SelectMatchPairs(self, matches, kp1_xy, kp2_xy, nMatch, width, height, gridX=3, gridY=3):
        """MosaicWithoutPos.cpp:4977-5028.  matches: DMATCH array (already sorted) or (n,2) int array."""
        matches = np.asarray(matches)
        if matches.dtype != DMATCH:
            mm = np.zeros(len(matches), DMATCH)
            mm["queryIdx"] = matches[:, 0]
            mm["trainIdx"] = matches[:, 1]
            matches = mm
        matches = np.ascontiguousarray(matches)
        kp1 = np.ascontiguousarray(kp1_xy, np.float32)
        kp2 = np.ascontiguousarray(kp2_xy, np.float32)
        v1 = np.zeros(400, SFPOINT)
        v2 = np.zeros(400, SFPOINT)
        n = C.c_int(0)
        self._chk(self.L.mi355_select_grid(self._h, _p(matches), len(matches), _p(kp1), len(kp1), _p(kp2), len(kp2), int(nMatch),
                                           int(width), int(height), int(gridX), int(gridY), _p(v1), _p(v2), C.byref(n)))
        return v1[:n.value].copy(), v2[:n.value].copy()

    def Ransac2D(self, p1, p2, fRansacDist=1.0, sampleTimes=1000, seed=1):
        """mosaicimage.h:1729-2035.  Returns (ok, inliers1, inliers2, H[9])."""
        p1 = np.ascontiguousarray(p1, SFPOINT)
        p2 = np.ascontiguousarray(p2, SFPOINT)
        n = len(p1)
        i1 = np.zeros(max(400, n), SFPOINT)
        i2 = np.zeros(max(400, n), SFPOINT)
        nin = C.c_int(0)
        H = np.zeros(9, np.float32)
        ok = self._chk(self.L.mi355_ransac2d(self._h, _p(p1), _p(p2), n, C.c_float(fRansacDist), int(sampleTimes), C.c_uint32(seed),
                                             _p(i1), _p(i2), C.byref(nin), _p(H)))
        return ok, i1[:nin.value].copy(), i2[:nin.value].copy(), H

    def ImageProjectionTransform(self, img, h9):
        """MosaicImage.cpp:1613-1758.  Returns (rows x widthStep u8 buffer, width, height, widthStep)."""
        img, w, h, ws, ch = _img_geom(img)
        h9 = np.ascontiguousarray(h9, np.float32)
        dst = C.c_void_p()
        dw, dh, dws = C.c_int(), C.c_int(), C.c_int()
        self._chk(self.L.mi355_warp_image(self._h, _p(img), w, h, ws, ch, _p(h9), C.byref(dst), C.byref(dw), C.byref(dh), C.byref(dws)))
        buf = _owned(self.L, dst, dh.value * dws.value, np.uint8).reshape(dh.value, dws.value)
        return buf, dw.value, dh.value, dws.value

    def MosaicImagesRefined(self, imgs, h9s, want_pixels=True):
        """CMosaicByPose::MosaicImagesRefined (float), MosaicWithoutPos.cpp:2194-2352.  want_pixels=False: the canvas the library returns is
        released without the numpy copy (bench.py times the C call, not this binding)."""
        return self._render_host(self.L.mi355_mosaic_refined, imgs, h9s, want_pixels=want_pixels)

    def MosaicImagesRefinedDev(self, d_imgs, w, h, ws, h9s, d_canvas, cw, ch, cws, row0=0, rows=-1):
        self._render_dev(self.L.mi355_mosaic_refined_dev, d_imgs, w, h, ws, h9s, (), d_canvas, cw, ch, cws, stripe=(row0, rows))

    # ---- SURF variant (GetMatchedPairsOneToAllSurf, MosaicWithoutPos.cpp:5300-5533) ---------------------
    def SurfExtract(self, img_id, bgr, hessian=50.0, max_kp=4096):
        img, w, h, ws, ch = _img_geom(bgr)
        assert ch == 3
        kp = np.zeros(max_kp, KEYPOINT)
        desc = np.zeros((max_kp, 128), np.float32)
        n = C.c_int(0)
        self._chk(self.L.mi355_surf_extract(self._h, int(img_id), _p(img), w, h, ws, C.c_float(hessian), int(max_kp), _p(kp), _p(desc), C.byref(n)))
        return kp[:n.value].copy(), desc[:n.value].copy()

    def SurfMatchPairs(self, pairs, ransac_dist=2.5, seed=1, match_dist=0.5, max_features=200, min_inliers=18):
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        out = np.zeros(len(pairs), PAIR_RESULT)
        self._chk(self.L.mi355_surf_match_pairs(self._h, _p(pairs), len(pairs), C.c_float(ransac_dist), C.c_uint32(seed), C.c_float(match_dist),
                                                int(max_features), int(min_inliers), _p(out)))
        return out

    # ---- multi-GPU exchanges -------------------------------------------------------------
    def PackFeaturesDev(self, img_ids, d_payload):
        """resident features of img_ids -> fixed-size records at d_payload (device, len x FEATURE_RECORD_BYTES); returns the headers"""
        ids = np.ascontiguousarray(img_ids, np.int32)
        hdr = np.zeros(len(ids), FEATURE_HEADER)
        self._chk(self.L.mi355_pack_features_dev(self._h, _p(ids), len(ids), _p(hdr), C.c_void_p(int(d_payload))))
        return hdr

    def InstallFeaturesDev(self, hdr, d_payload):
        hdr = np.ascontiguousarray(hdr, FEATURE_HEADER)
        self._chk(self.L.mi355_install_features_dev(self._h, _p(hdr), C.c_void_p(int(d_payload)), len(hdr)))

    def FeatureChunkCount(self, img_ids):
        """the chunk records the resident features of img_ids take (sum of max(1, ceil(n_kp / 2048)))"""
        ids = np.ascontiguousarray(img_ids, np.int32)
        n = C.c_int(0)
        self._chk(self.L.mi355_feature_chunk_count(self._h, _p(ids), len(ids), C.byref(n)))
        return n.value

    def PackFeatureChunksDev(self, img_ids, d_payload, max_records):
        """resident features of img_ids (any keypoint count) -> chunk records at d_payload (device, max_records x FEATURE_RECORD_BYTES);
        returns the FEATURE_CHUNK_HEADER array of the records written"""
        ids = np.ascontiguousarray(img_ids, np.int32)
        hdr = np.zeros(max(int(max_records), 1), FEATURE_CHUNK_HEADER)
        n = C.c_int(0)
        self._chk(self.L.mi355_pack_feature_chunks_dev(self._h, _p(ids), len(ids), _p(hdr), C.c_void_p(int(d_payload) or None), int(max_records), C.byref(n)))
        return hdr[:n.value].copy()

    def InstallFeatureChunksDev(self, hdr, d_payload):
        """chunk records -> resident features (the whole table is checked first: a bad one raises and changes nothing)"""
        hdr = np.ascontiguousarray(hdr, FEATURE_CHUNK_HEADER)
        self._chk(self.L.mi355_install_feature_chunks_dev(self._h, _p(hdr), C.c_void_p(int(d_payload) or None), len(hdr)))

    def CompactAcceptedDev(self, d_in, n, d_out):
        k = C.c_int(0)
        self._chk(self.L.mi355_compact_accepted_dev(self._h, C.c_void_p(int(d_in)), int(n), C.c_void_p(int(d_out)), C.byref(k)))
        return k.value

    def last_sift_counters(self):
        """SIFT stage populations of the last extracted frame: DoG extrema, refined points, oriented keypoints, kept, overflow flag"""
        out = (C.c_int32 * 8)()
        self._chk(self.L.mi355_last_sift_counters(self._h, out))
        return list(out)

    def CommInit(self, id128, rank, world):
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(id128))
        self._chk(self.L.mi355_comm_init(self._h, buf, int(rank), int(world)))

    def CommDestroy(self):
        self._chk(self.L.mi355_comm_destroy(self._h))

    def CommInfo(self):
        """(rank, n_ranks) as the RCCL communicator itself reports them (ncclCommUserRank / ncclCommCount)"""
        r, n = C.c_int(0), C.c_int(0)
        self._chk(self.L.mi355_comm_info(self._h, C.byref(r), C.byref(n)))
        return r.value, n.value

    def AllGatherFeatures(self, img_ids, n_max_per_rank):
        ids = np.ascontiguousarray(img_ids, np.int32)
        self._chk(self.L.mi355_allgather_features(self._h, _p(ids), len(ids), int(n_max_per_rank)))

    def AllGatherFeatureChunks(self, img_ids, install_own=False):
        """mi355_allgather_feature_chunks: the features of every rank's frames, any keypoint count, resident on every rank afterwards.
        install_own: this rank's own frames are re-installed from the received records too."""
        ids = np.ascontiguousarray(img_ids, np.int32)
        self._chk(self.L.mi355_allgather_feature_chunks(self._h, _p(ids), len(ids), 1 if install_own else 0))

    def AllGatherResults(self, d_local, n_local, accepted_only=True, root=-1, copy=True, wait=True):
        """mi355_allgather_results.  root < 0: every rank receives all ranks' records; root >= 0: only that rank (the others send and
        get an empty array).  The library hands out a view of pinned memory it owns, valid until the next call: copy=True (default)
        returns a private numpy copy, copy=False the view itself (bench.py: a 1.1 GB numpy copy per step would be the measurement).
        wait=False (root >= 0, copy=False): MI355_GATHER_NO_WAIT -- the view is complete after the next synchronize()."""
        assert wait or (root >= 0 and not copy)
        ptr, n = C.c_void_p(), C.c_int(0)
        flags = (1 if accepted_only else 0) | (0 if wait else 2)
        self._chk(self.L.mi355_allgather_results(self._h, C.c_void_p(int(d_local)), int(n_local), flags, int(root), C.byref(ptr), C.byref(n)))
        return _owned(self.L, ptr, n.value, PAIR_RESULT, copy=copy, free=False)

    def PairMomentsDev(self, d_results, n, d_out):
        """one PAIR_MOMENTS record per pair record, device to device (ctx stream)"""
        self._chk(self.L.mi355_pair_moments_dev(self._h, C.c_void_p(int(d_results)), int(n), C.c_void_p(int(d_out))))

    def PairNormalBlocksDev(self, d_results, n, h8, part, d_out):
        """one PAIR_NORMAL_BLOCK per pair record at the parameters h8 (n_images x 8 doubles, host) and flags part (n_images bytes, host:
        0 no part, 1 takes part, 2 fixed), device to device (ctx stream)"""
        h8 = np.ascontiguousarray(h8, np.float64).reshape(-1, 8)
        part = np.ascontiguousarray(part, np.uint8)
        assert len(h8) == len(part)
        self._chk(self.L.mi355_pair_normal_blocks_dev(self._h, C.c_void_p(int(d_results)), int(n), _p(h8), _p(part), len(part), C.c_void_p(int(d_out))))

    def GlobalProjectiveRefineDev(self, d_results, n_pairs, w, h, start, fixed=None, label=None, params=None):
        """mi355_global_projective_refine_dev: the projective refinement of `start` on device records; returns (transforms, report dict)"""
        a = _projective_args(w, h, start, fixed, label)
        out, rep = np.zeros(len(a[2]), IMAGE_TRANSFORM), ProjectiveReport()
        self._chk(self.L.mi355_global_projective_refine_dev(self._h, C.c_void_p(int(d_results) or None), int(n_pairs), len(a[2]), _p(a[0]), _p(a[1]), _p(a[3]), _p(a[4]), _p(a[2]),
                                                            _ref(params), _p(out), C.byref(rep)))
        return out, rep.as_dict()

    # ---- lens self-calibration (mi355_pair_calib_blocks_dev, mi355_calibrate_lens_dev; csrc/calib.hip) --------------------------
    def PairCalibBlocksDev(self, d_results, n, h8, cam, d_out, min_ties=16):
        """one PAIR_CALIB_BLOCK per pair record at the camera `cam` (Camera: its coefficients are theta) and the states h8 (n x 8 doubles,
        one row per record, host), device to device (ctx stream)"""
        h8 = None if h8 is None else np.ascontiguousarray(h8, np.float64).reshape(-1, 8)
        assert h8 is None or len(h8) >= int(n)
        self._chk(self.L.mi355_pair_calib_blocks_dev(self._h, _dptr(d_results), int(n), _p(h8), _ref(cam),
                                                     int(min_ties), _dptr(d_out)))

    def CalibrateLensDev(self, d_results, n_pairs, start, params=None, **kw):
        """mi355_calibrate_lens_dev: the Brown-Conrady coefficients of the camera `start` (Camera; its intrinsics are held fixed) from device
        pair records of the original frames; returns (Camera, report dict)"""
        p = _resolve(params, calib_params, kw)
        out, rep = Camera(), CalibReport()
        self._chk(self.L.mi355_calibrate_lens_dev(self._h, _dptr(d_results), int(n_pairs), _ref(start), C.byref(p),
                                                  C.byref(out), C.byref(rep)))
        return out, rep.as_dict()

    # ---- tie-point refinement (mi355_refine_ties*, csrc/tie_refine.hip) ------------------------------------------------------
    def RefineTiesDev(self, d_in, n, d_imgs, w, h, ws, d_out, d_status=0, d_ncc2=0, d_report=0, params=None, **kw):
        """mi355_refine_ties_dev: n device pair records d_in -> d_out (may be d_in) with every inlier's position in image i moved to the
        correlation peak of the patch around its partner in image j.  d_imgs: device frames (0 / None: not held), w, h, ws their geometry;
        d_status (uint8 [n, 400]), d_ncc2 (float32 [n, 400]), d_report (TIE_REPORT [n]): device buffers, 0 = not wanted.  params: TieParams
        (tie_params()) or its keyword fields (radius, search, drop_mask, min_ncc).  Enqueued on the ctx stream."""
        n_img, ptrs, w, h, ws, _ = _dev_frames(d_imgs, w, h, ws)
        p = _resolve(params, tie_params, kw)
        self._chk(self.L.mi355_refine_ties_dev(self._h, _dptr(d_in), int(n), ptrs, _p(w), _p(h), _p(ws), n_img, C.byref(p),
                                               _dptr(d_out), _dptr(d_status),
                                               _dptr(d_ncc2), _dptr(d_report)))

    def RefineTies(self, results, imgs, img_ids=None, geom=None, params=None, **kw):
        """mi355_refine_ties: host PAIR_RESULT records in; image k from the kept frame of img_ids[k] (>= 0) or from the host image imgs[k]
        (None: not held).  Returns (results, status uint8 [n, 400], ncc2 float32 [n, 400], report TIE_REPORT [n])."""
        res = np.ascontiguousarray(results, PAIR_RESULT)
        n = len(res)
        ptrs, ids, w, h, ws, _keep = self._into_args(imgs, img_ids, geom)
        p = _resolve(params, tie_params, kw)
        out = np.zeros(n, PAIR_RESULT)
        status, ncc2, report = np.zeros((n, 400), np.uint8), np.zeros((n, 400), np.float32), np.zeros(n, TIE_REPORT)
        self._chk(self.L.mi355_refine_ties(self._h, _p(res), n, ptrs, _p(ids), _p(w), _p(h), _p(ws), len(ids), C.byref(p), _p(out), _p(status), _p(ncc2),
                                           _p(report)))
        return out, status, ncc2, report

    def AllGatherMoments(self, d_local, n_local, copy=True):
        """this rank's accepted pairs -> their second moments -> every rank's host (rank-major PAIR_MOMENTS array; pinned memory of the
        library, see AllGatherResults for `copy`)"""
        ptr, n = C.c_void_p(), C.c_int(0)
        self._chk(self.L.mi355_allgather_moments(self._h, C.c_void_p(int(d_local)), int(n_local), C.byref(ptr), C.byref(n)))
        return _owned(self.L, ptr, n.value, PAIR_MOMENTS, copy=copy, free=False)

    def StripeCover(self, w, h, h9s, row0, rows, blended=False, keep=None, band=5, exact=False):
        """mi355_mosaic_stripe_cover: need[k] = 1 when rendering canvas rows [row0, row0 + rows) reads frame k.  exact (refined canvas only): the
        frames that give at least one pixel its sample (a device pass), instead of every frame whose box meets the rows"""
        keep_a = _arr(keep, np.uint8)
        mode = 1 if blended else (2 if exact else 0)
        return self._render_cover(self.L.mi355_mosaic_stripe_cover, w, h, h9s, (_p(keep_a), int(band)), row0, rows, first=(mode,))

    def ExchangeFrames(self, d_frames, h, ws, need, owner=None, own_through_rccl=False):
        """mi355_exchange_frames.  d_frames: per frame this rank's device pointer (0 / None where it does not hold the frame); need: [G, n]
        uint8 table (the same on every rank), or [n]: this rank's own row (the rows are all-gathered inside the call).  Returns (pointers for
        the stripe calls -- 0 where the rank's stripe does not read the frame --, bytes received, bytes sent)."""
        n = len(d_frames)
        ptrs = _dptrs(d_frames, 1)
        h = np.ascontiguousarray(h, np.int32); ws = np.ascontiguousarray(ws, np.int32)
        need = np.ascontiguousarray(need, np.uint8)
        local = need.ndim == 1
        assert need.shape[-1] == n
        own_a = _arr(owner, np.int32)
        out = (C.c_void_p * max(n, 1))()
        br, bs = C.c_uint64(0), C.c_uint64(0)
        flags = (1 if own_through_rccl else 0) | (2 if local else 0)
        self._chk(self.L.mi355_exchange_frames(self._h, ptrs, _p(h), _p(ws), n, _p(own_a), _p(need), flags, out, C.byref(br), C.byref(bs)))
        return [int(out[k] or 0) for k in range(n)], int(br.value), int(bs.value)

    def SynthFrameDev(self, d_dst, w, h, ws, A6, seed, frame_seed, gain=1.0, noise=2.0):
        A6 = np.ascontiguousarray(A6, np.float32)
        self._chk(self.L.mi355_synth_frame_dev(self._h, C.c_void_p(int(d_dst)), int(w), int(h), int(ws), _p(A6), C.c_uint32(seed),
                                               C.c_uint32(frame_seed), C.c_float(gain), C.c_float(noise)))

    def ChipsAndMasks(self, imgs, h9s, keep=None, find_masks=True):
        """LaplacianPyramidBlending warp stage + FindMasksByDistMap (MosaicImage.cpp:2233-2460, 1761-1881)."""
        n, imgs, ptrs, w, h, ws = _host_frames(imgs)
        h9s, keep_a = _arr(h9s, np.float32), _arr(keep, np.uint8)
        return self._chips(self.L.mi355_chips_and_masks, ptrs, _p(w), _p(h), _p(ws), n, _p(h9s), _p(keep_a), int(bool(find_masks)))

    def MultiBandBlend(self, chips, chip_imgs, masks, cw, ch, band=5):
        """detail::MultiBandBlender(false, band) over the chips of ChipsAndMasks (MosaicImage.cpp:2296-2299, 2451-2486)."""
        n = len(chip_imgs)
        ci = [np.ascontiguousarray(c, np.uint8) for c in chip_imgs]
        mi = [np.ascontiguousarray(m, np.uint8) for m in masks]
        cp = (C.c_void_p * max(n, 1))(*[c.ctypes.data for c in ci])
        mp = (C.c_void_p * max(n, 1))(*[m.ctypes.data for m in mi])
        info = np.ascontiguousarray(chips, CHIPINFO)
        out = C.c_void_p()
        ow, oh, ows = C.c_int(), C.c_int(), C.c_int()
        self._chk(self.L.mi355_multiband_blend(self._h, cp, mp, _p(info), n, int(cw), int(ch), int(band), C.byref(out), C.byref(ow), C.byref(oh), C.byref(ows)))
        buf = _owned(self.L, out, ows.value * oh.value, np.uint8).reshape(oh.value, ows.value)
        return buf, ow.value, oh.value, ows.value

    def MosaicBlended(self, imgs, h9s, keep=None, band=5):
        """LaplacianPyramidBlending in one call (MosaicImage.cpp:2205-2510): chips, masks and blend stay on the device."""
        keep_a = _arr(keep, np.uint8)
        return self._render_host(self.L.mi355_mosaic_blended, imgs, h9s, (_p(keep_a), int(band)))

    def MosaicBlendedDev(self, d_ptrs, w, h, ws, h9s, keep=None, band=5, row0=0, rows=-1):
        """LaplacianPyramidBlending with the survey resident in HBM: device frames in, device canvas out (a torch uint8 tensor
        [ch, cws]); chips, masks and the blender's pyramids stay in the ctx's buffers.
        Ordering: the library writes the canvas on the ctx's stream, the tensor comes from torch's allocator (torch's current stream).  The
        wrapper synchronises torch's stream before the call (a recycled block may still be in use by pending torch work) and the ctx's
        stream after it: the tensor it returns is complete and safe to use on any stream."""
        import torch
        n, ptrs, w, h, ws, h9s = _dev_frames(d_ptrs, w, h, ws, h9s)
        keep_a = _arr(keep, np.uint8)
        cw, ch, cws = blend_layout(w, h, h9s, keep_a)
        if rows >= 0:
            # one stripe of the canvas (a rank's share): the tensor holds the rows row0 .. row0 + rows - 1; cw, ch, cws stay the whole canvas's
            out = torch.empty((rows, cws), dtype=torch.uint8, device=torch.device("cuda", self.device))
            torch.cuda.current_stream(out.device).synchronize()
            self._chk(self.L.mi355_mosaic_blended_rows_dev(self._h, ptrs, _p(w), _p(h), _p(ws), n, _p(h9s), _p(keep_a), int(band),
                                                           C.c_void_p(out.data_ptr()), cw, ch, cws, int(row0), int(rows)))
            self.synchronize()
            return out, cw, ch, cws
        out = torch.empty((ch, cws), dtype=torch.uint8, device=torch.device("cuda", self.device))
        torch.cuda.current_stream(out.device).synchronize()
        self._chk(self.L.mi355_mosaic_blended_dev(self._h, ptrs, _p(w), _p(h), _p(ws), n, _p(h9s), _p(keep_a), int(band),
                                                  C.c_void_p(out.data_ptr()), cw, ch, cws))
        self.synchronize()
        return out, cw, ch, cws

    # ---- exposure gain compensation (mi355_gain_*, csrc/gain.hip) ----------------------------------------------------------
    @staticmethod
    def _pairs_ab(pairs):
        ab = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
        return ab, len(ab)

    def GainStatsDev(self, d_imgs, w, h, ws, h9s, pairs, step=8):
        """overlap statistics of the listed pairs (positions in the frame list) on the lattice of `step`: (GAIN_PAIR_STATS [n_pairs],
        frame cover N_k int64 [n])"""
        n, ptrs, w, h, ws, h9s = _dev_frames(d_imgs, w, h, ws, h9s)
        ab, npairs = self._pairs_ab(pairs)
        st = np.zeros(npairs, GAIN_PAIR_STATS)
        cover = np.zeros(n, np.int64)
        self._chk(self.L.mi355_gain_stats_dev(self._h, ptrs, _p(w), _p(h), _p(ws), n, _p(h9s), _p(ab), npairs, int(step), _p(st), _p(cover)))
        return st, cover

    def ApplyGainsDev(self, d_src, d_dst, w, h, ws, gains):
        """d_dst[k] = LUT_k(d_src[k]) (d_dst[k] may be d_src[k]); gains [n, 3] float32.  Complete on return."""
        n, sp, w, h, ws, _ = _dev_frames(d_src, w, h, ws)
        dp = _dptrs(d_dst, n)
        g = np.ascontiguousarray(gains, np.float32).reshape(n, 3)
        self._chk(self.L.mi355_apply_gains_dev(self._h, sp, dp, _p(w), _p(h), _p(ws), n, _p(g)))

    def GainCompensateDev(self, d_imgs, w, h, ws, h9s, pairs, params=None, **kw):
        """statistics, solve and in-place apply on the device frames; returns the gains [n, 3] float32.  params: GainParams (gain_params())
        or keyword fields of it."""
        n, ptrs, w, h, ws, h9s = _dev_frames(d_imgs, w, h, ws, h9s)
        ab, npairs = self._pairs_ab(pairs)
        p = _resolve(params, gain_params, kw)
        g = np.zeros((n, 3), np.float32)
        self._chk(self.L.mi355_gain_compensate_dev(self._h, ptrs, _p(w), _p(h), _p(ws), n, _p(h9s), _p(ab), npairs, C.byref(p), _p(g)))
        return g

    # ---- frame sharpness (mi355_sharp_*, csrc/sharp.hip) ---------------------------------------------------------------------
    def SharpStatsDev(self, d_imgs, w, h, ws, h9s, pairs, step=8, frames=True):
        """Laplacian statistics of the listed pairs (positions in the frame list) on the lattice of `step`: (SHARP_PAIR_STATS [n_pairs],
        SHARP_FRAME_STATS [n], or None with frames=False: then no per-frame tiles are launched)"""
        n, ptrs, w, h, ws, h9s = _dev_frames(d_imgs, w, h, ws, h9s)
        ab, npairs = self._pairs_ab(pairs)
        st = np.zeros(npairs, SHARP_PAIR_STATS)
        fs = np.zeros(n, SHARP_FRAME_STATS) if frames else None
        self._chk(self.L.mi355_sharp_stats_dev(self._h, ptrs, _p(w), _p(h), _p(ws), n, _p(h9s), _p(ab), npairs, int(step), _p(st),
                                               _p(fs) if frames else None))
        return st, fs

    def SharpnessDev(self, d_imgs, w, h, ws, h9s, pairs, params=None, **kw):
        """statistics, solve, flag and select on the device frames (which are only read): (sharp [n] float32, status [n] uint8, h9s_kept
        [n, 9] float32 -- h9s with m8 = 0 for the dropped frames, status 1).  params: SharpParams (sharp_params()) or keyword fields of it."""
        n, ptrs, w, h, ws, h9s = _dev_frames(d_imgs, w, h, ws, h9s)
        ab, npairs = self._pairs_ab(pairs)
        p = _resolve(params, sharp_params, kw)
        sharp = np.zeros(n, np.float32)
        status = np.zeros(n, np.uint8)
        self._chk(self.L.mi355_sharpness_dev(self._h, ptrs, _p(w), _p(h), _p(ws), n, _p(h9s), _p(ab), npairs, C.byref(p), _p(sharp), _p(status)))
        return sharp, status, drop_sharp_frames(h9s, status)

    # ---- cover depth (mi355_cover_*, csrc/cover.hip) ----------------------------------------------------------------------------
    def CoverStatsDev(self, w, h, h9s, keep=None, step=8):
        """how deep the kept frames cover the canvas lattice of `step` (geometry only, no images): (COVER_FRAME_STATS [n], hist int64
        [COVER_BINS]).  keep: n bytes, None = every frame."""
        w, h, h9s, n, keep = _cover_args(w, h, h9s, keep)
        fs = np.zeros(n, COVER_FRAME_STATS)
        hist = np.zeros(COVER_BINS, np.int64)
        self._chk(self.L.mi355_cover_stats_dev(self._h, _p(w), _p(h), n, _p(h9s), _p(keep), int(step), _p(fs), _p(hist)))
        return fs, hist

    def CoverSelectDev(self, w, h, h9s, order=None, pairs=None, keep=None, params=None, final=False, **kw):
        """coverage-checked frame dropping with the kernel as the statistics of every round: (status [n] uint8 -- 0 not a candidate, 1
        dropped, 2 kept for coverage, 3 kept as a cut vertex, 4 not examined --, keep_out [n] uint8, rounds, lost) and, with final=True, the
        (COVER_FRAME_STATS [n], hist) under keep_out.  order: candidate positions by priority, None = every kept frame by ascending crit;
        pairs: the graph that must stay connected, None = no connectivity check; params: CoverParams (cover_params()) or keyword fields."""
        w, h, h9s, n, keep = _cover_args(w, h, h9s, keep)
        order, n_order, ab, npairs = _cover_lists(order, pairs)
        p = _resolve(params, cover_params, kw)
        status, keep_out = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        rounds, lost = C.c_int32(0), C.c_int64(0)
        fs = np.zeros(n, COVER_FRAME_STATS) if final else None
        hist = np.zeros(COVER_BINS, np.int64) if final else None
        self._chk(self.L.mi355_cover_select_dev(self._h, _p(w), _p(h), n, _p(h9s), _p(keep), _p(order), n_order, _p(ab), npairs, C.byref(p),
                                                _p(status), _p(keep_out), C.byref(rounds), C.byref(lost), _p(fs), _p(hist)))
        out = (status, keep_out, int(rounds.value), int(lost.value))
        return out + (fs, hist) if final else out

    # ---- block gain compensation (mi355_block_gain_*, csrc/gain.hip) -------------------------------------------------------
    def BlockGainStatsDev(self, d_imgs, w, h, ws, h9s, pairs, step=8, grid_x=8, grid_y=6):
        """per-cell overlap statistics of the listed pairs: (BLOCK_GAIN_STATS records sorted by (pair, cell_a, cell_b), cell cover int64
        [n, grid_y * grid_x])"""
        n, ptrs, w, h, ws, h9s = _dev_frames(d_imgs, w, h, ws, h9s)
        ab, npairs = self._pairs_ab(pairs)
        cover = np.zeros((n, max(int(grid_x) * int(grid_y), 0)), np.int64)
        recs, nrec = C.c_void_p(), C.c_int64(0)
        self._chk(self.L.mi355_block_gain_stats_dev(self._h, ptrs, _p(w), _p(h), _p(ws), n, _p(h9s), _p(ab), npairs, int(step), int(grid_x), int(grid_y),
                                                    C.byref(recs), C.byref(nrec), _p(cover)))
        return _owned(self.L, recs, nrec.value, BLOCK_GAIN_STATS), cover

    def ApplyBlockGainsDev(self, d_src, d_dst, w, h, ws, gains):
        """d_dst[k] = d_src[k] times its interpolated gain map (d_dst[k] may be d_src[k]); gains [n, grid_y, grid_x, 3] float32.  Complete
        on return."""
        n, sp, w, h, ws, _ = _dev_frames(d_src, w, h, ws)
        dp = _dptrs(d_dst, n)
        g = np.ascontiguousarray(gains, np.float32)
        if g.ndim != 4 or g.shape[0] != n or g.shape[3] != 3:
            raise ValueError("gains must be [n, grid_y, grid_x, 3]")
        self._chk(self.L.mi355_apply_block_gains_dev(self._h, sp, dp, _p(w), _p(h), _p(ws), n, int(g.shape[2]), int(g.shape[1]), _p(g)))

    def BlockGainCompensateDev(self, d_imgs, w, h, ws, h9s, pairs, params=None, **kw):
        """statistics, solve, smoothing and in-place apply on the device frames; returns the gain maps [n, grid_y, grid_x, 3] float32.
        params: BlockGainParams (block_gain_params()) or keyword fields of it."""
        n, ptrs, w, h, ws, h9s = _dev_frames(d_imgs, w, h, ws, h9s)
        ab, npairs = self._pairs_ab(pairs)
        p = _resolve(params, block_gain_params, kw)
        g = np.zeros((n, max(p.grid_y, 0), max(p.grid_x, 0), 3), np.float32)
        if g.size > (1 << 28):
            g = np.zeros((n, 1, 1, 3), np.float32)                # a grid the library refuses
        self._chk(self.L.mi355_block_gain_compensate_dev(self._h, ptrs, _p(w), _p(h), _p(ws), n, _p(h9s), _p(ab), npairs, C.byref(p), _p(g)))
        return g

    # ---- weighted (feather) blending (mi355_mosaic_feathered*, csrc/feather.hip) -------------------------------------------
    def MosaicFeathered(self, imgs, h9s, params=None, want_pixels=True, **kw):
        """mi355_mosaic_feathered: host images in, (canvas rows x cws, cw, ch, cws) out.  params: FeatherParams (feather_params()) or its
        keyword fields (ramp)."""
        p = _resolve(params, feather_params, kw)
        return self._render_host(self.L.mi355_mosaic_feathered, imgs, h9s, (C.byref(p),), want_pixels=want_pixels)

    def MosaicFeatheredDev(self, d_imgs, w, h, ws, h9s, d_canvas, cw, ch, cws, row0=0, rows=-1, params=None, **kw):
        """mi355_mosaic_feathered_dev: device frames (0 / None: withheld) into the device canvas, rows [row0, row0 + rows); complete on return"""
        p = _resolve(params, feather_params, kw)
        self._render_dev(self.L.mi355_mosaic_feathered_dev, d_imgs, w, h, ws, h9s, (C.byref(p),), d_canvas, cw, ch, cws, stripe=(row0, rows))

    def MosaicFeatheredInto(self, imgs, img_ids, h9s, out=None, pitch=None, geom=None, params=None, **kw):
        """mi355_mosaic_feathered_into, sources and destination as MosaicImagesRefinedInto.  Returns (out, cw, ch)."""
        p = _resolve(params, feather_params, kw)
        return self._render_into(self.L.mi355_mosaic_feathered_into, imgs, img_ids, h9s, (C.byref(p),), mosaic_layout, out, pitch, geom)

    # ---- seamline render (mi355_mosaic_seamline*, csrc/seamline.hip) -------------------------------------------------------
    def MosaicSeamline(self, imgs, h9s, params=None, want_owner=False, **kw):
        """mi355_mosaic_seamline: host images in, (canvas rows x cws, cw, ch, cws) out -- with want_owner (canvas, cw, ch, cws, owner [ch, cw]
        uint16: owning frame + 1, 0 where nothing covers).  params: SeamlineParams (seamline_params()) or its keyword fields (ramp)."""
        p = _resolve(params, seamline_params, kw)
        return self._render_host(self.L.mi355_mosaic_seamline, imgs, h9s, (C.byref(p),), extra=(want_owner, np.uint16))

    def MosaicSeamlineDev(self, d_imgs, w, h, ws, h9s, d_canvas, cw, ch, cws, row0=0, rows=-1, d_owner=0, d_count=0, params=None, **kw):
        """mi355_mosaic_seamline_dev: device frames (0 / None: withheld; d_imgs None when d_canvas is 0) into the device canvas and / or the
        uint16 [ch, cw] maps d_owner, d_count (0: not wanted), rows [row0, row0 + rows); complete on return"""
        p = _resolve(params, seamline_params, kw)
        self._render_dev(self.L.mi355_mosaic_seamline_dev, d_imgs, w, h, ws, h9s, (C.byref(p),), d_canvas, cw, ch, cws, maps=(d_owner, d_count),
                         stripe=(row0, rows))

    def MosaicSeamlineInto(self, imgs, img_ids, h9s, out=None, pitch=None, geom=None, params=None, **kw):
        """mi355_mosaic_seamline_into, sources and destination as MosaicImagesRefinedInto.  Returns (out, cw, ch)."""
        p = _resolve(params, seamline_params, kw)
        return self._render_into(self.L.mi355_mosaic_seamline_into, imgs, img_ids, h9s, (C.byref(p),), mosaic_layout, out, pitch, geom)

    def SeamlineCover(self, w, h, h9s, row0=0, rows=-1, params=None, **kw):
        """mi355_mosaic_seamline_cover: need[k] = 1 exactly for the frames that own at least one pixel of canvas rows [row0, row0 + rows)"""
        p = _resolve(params, seamline_params, kw)
        return self._render_cover(self.L.mi355_mosaic_seamline_cover, w, h, h9s, (C.byref(p),), row0, rows)

    # ---- optimised seamlines (mi355_seam_*, mi355_mosaic_seamcut*, csrc/seamcut.hip) ------------------------------------------
    def SeamCandidatesDev(self, d_imgs, w, h, ws, h9s, d_cand, gw, gh, params=None, **kw):
        """mi355_seam_candidates_dev: the cell records (SEAM_CELL, 32 bytes each) of the gh x gw grid into device memory d_cand"""
        n, ptrs, w, h, ws, h9s = _dev_frames(d_imgs, w, h, ws, h9s)
        p = _resolve(params, seamcut_params, kw)
        self._chk(self.L.mi355_seam_candidates_dev(self._h, ptrs, _p(w), _p(h), _p(ws), n, _p(h9s), C.byref(p), _dptr(d_cand),
                                                   int(gw), int(gh)))

    def SeamLabelsDev(self, d_cand, gw, gh, d_cells, params=None, **kw):
        """mi355_seam_labels_dev: device records in, the uint16 [gh, gw] cell map into device memory d_cells; returns the report dict"""
        p = _resolve(params, seamcut_params, kw)
        r = SeamReport()
        self._chk(self.L.mi355_seam_labels_dev(self._h, _dptr(d_cand), int(gw), int(gh), C.byref(p),
                                               _dptr(d_cells), C.byref(r)))
        return _report(r)

    def SeamCellsDev(self, d_imgs, w, h, ws, h9s, d_cells, gw, gh, params=None, **kw):
        """mi355_seam_cells_dev: candidates and labels in one call; returns the report dict"""
        n, ptrs, w, h, ws, h9s = _dev_frames(d_imgs, w, h, ws, h9s)
        p = _resolve(params, seamcut_params, kw)
        r = SeamReport()
        self._chk(self.L.mi355_seam_cells_dev(self._h, ptrs, _p(w), _p(h), _p(ws), n, _p(h9s), C.byref(p), _dptr(d_cells),
                                              int(gw), int(gh), C.byref(r)))
        return _report(r)

    def MosaicSeamCutDev(self, d_imgs, w, h, ws, h9s, d_canvas, cw, ch, cws, row0=0, rows=-1, d_cells=0, d_owner=0, d_count=0, params=None, **kw):
        """mi355_mosaic_seamcut_dev: the seamline render following the device cell map d_cells (0: candidates and labels are made first, all
        three stages in one call); outputs, stripes and withheld frames as MosaicSeamlineDev; complete on return"""
        p = _resolve(params, seamcut_params, kw)
        self._render_dev(self.L.mi355_mosaic_seamcut_dev, d_imgs, w, h, ws, h9s, (C.byref(p), _dptr(d_cells)), d_canvas, cw, ch, cws,
                         maps=(d_owner, d_count), stripe=(row0, rows))

    def MosaicSeamCut(self, imgs, h9s, params=None, want_owner=False, **kw):
        """mi355_mosaic_seamcut: host images in, all three stages, outputs as MosaicSeamline"""
        p = _resolve(params, seamcut_params, kw)
        return self._render_host(self.L.mi355_mosaic_seamcut, imgs, h9s, (C.byref(p),), extra=(want_owner, np.uint16))

    def MosaicSeamCutInto(self, imgs, img_ids, h9s, out=None, pitch=None, geom=None, params=None, **kw):
        """mi355_mosaic_seamcut_into, sources and destination as MosaicImagesRefinedInto.  Returns (out, cw, ch)."""
        p = _resolve(params, seamcut_params, kw)
        return self._render_into(self.L.mi355_mosaic_seamcut_into, imgs, img_ids, h9s, (C.byref(p),), mosaic_layout, out, pitch, geom)

    def SeamCutCover(self, w, h, h9s, d_cells, row0=0, rows=-1, params=None, **kw):
        """mi355_mosaic_seamcut_cover: need[k] = 1 exactly for the frames that own a pixel of canvas rows [row0, row0 + rows) under d_cells"""
        p = _resolve(params, seamcut_params, kw)
        return self._render_cover(self.L.mi355_mosaic_seamcut_cover, w, h, h9s, (C.byref(p), _dptr(d_cells)), row0, rows)

    # ---- multiband blend along optimised seams (mi355_blend_seam_*, mi355_*_seam*, csrc/blend_seam.hip) ------------------------
    def BlendSeamCellsDev(self, d_imgs, w, h, ws, h9s, d_cells, gw, gh, keep=None, d_cand=0, params=None, **kw):
        """mi355_blend_seam_cells_dev: candidates (in the blend's geometry) and labels; the uint16 [gh, gw] cell map into device memory
        d_cells, the records into d_cand when given; returns the report dict"""
        n, ptrs, w, h, ws, h9s = _dev_frames(d_imgs, w, h, ws, h9s)
        p = _resolve(params, seamcut_params, kw)
        keep_a = _arr(keep, np.uint8)
        r = SeamReport()
        self._chk(self.L.mi355_blend_seam_cells_dev(self._h, ptrs, _p(w), _p(h), _p(ws), n, _p(h9s), _p(keep_a), C.byref(p),
                                                    _dptr(d_cells), int(gw), int(gh), C.byref(r), _dptr(d_cand)))
        return _report(r)

    def ChipsAndMasksSeam(self, imgs, h9s, keep=None, cells=None, params=None, **kw):
        """mi355_chips_and_masks_seam: ChipsAndMasks(find_masks=True) whose ownership follows the host cell map `cells` ([gh, gw] uint16;
        None: candidates and labels are made first).  The same dictionary; feeds MultiBandBlend."""
        n, imgs, ptrs, w, h, ws = _host_frames(imgs)
        h9s, keep_a = _arr(h9s, np.float32), _arr(keep, np.uint8)
        p = _resolve(params, seamcut_params, kw)
        if cells is None:
            gw, gh = blend_seam_grid(w, h, h9s, p.level, keep_a)
        else:
            cells = np.ascontiguousarray(cells, np.uint16)
            gh, gw = cells.shape
        return self._chips(self.L.mi355_chips_and_masks_seam, ptrs, _p(w), _p(h), _p(ws), n, _p(h9s), _p(keep_a), C.byref(p), _p(cells),
                           int(gw), int(gh))

    def MosaicBlendedSeamDev(self, d_imgs, w, h, ws, h9s, d_canvas, cw, ch, cws, keep=None, band=5, d_cells=0, gw=None, gh=None, params=None, **kw):
        """mi355_mosaic_blended_seam_dev: device frames in, the blended canvas into device memory d_canvas; the ownership follows the device
        cell map d_cells (0: it is made first).  Enqueued on the ctx's stream and waited for."""
        p = _resolve(params, seamcut_params, kw)
        keep_a = _arr(keep, np.uint8)
        if gw is None or gh is None:
            gw, gh = blend_seam_grid(w, h, h9s, p.level, keep_a)
        self._render_dev(self.L.mi355_mosaic_blended_seam_dev, d_imgs, w, h, ws, h9s,
                         (_p(keep_a), int(band), C.byref(p), _dptr(d_cells), int(gw), int(gh)), d_canvas, cw, ch, cws)
        self.synchronize()

    def MosaicBlendedSeam(self, imgs, h9s, keep=None, band=5, params=None, **kw):
        """mi355_mosaic_blended_seam: host images in, all three stages and the blend; outputs as MosaicBlended"""
        keep_a = _arr(keep, np.uint8)
        p = _resolve(params, seamcut_params, kw)
        return self._render_host(self.L.mi355_mosaic_blended_seam, imgs, h9s, (_p(keep_a), int(band), C.byref(p)))

    def MosaicBlendedSeamInto(self, imgs, img_ids, h9s, keep=None, band=5, out=None, pitch=None, geom=None, params=None, **kw):
        """mi355_mosaic_blended_seam_into, sources and destination as MosaicBlendedInto.  Returns (out, cw, ch)."""
        keep_a = _arr(keep, np.uint8)
        p = _resolve(params, seamcut_params, kw)
        return self._render_into(self.L.mi355_mosaic_blended_seam_into, imgs, img_ids, h9s, (_p(keep_a), int(band), C.byref(p)),
                                 lambda w, h, h9s: blend_layout(w, h, h9s, keep_a), out, pitch, geom)

    # ---- median render (mi355_mosaic_median*, csrc/median.hip) -------------------------------------------------------------
    def MosaicMedian(self, imgs, h9s, params=None, want_spread=False, **kw):
        """mi355_mosaic_median: host images in, (canvas rows x cws, cw, ch, cws) out -- with want_spread (canvas, cw, ch, cws, spread [ch, cw]
        uint8: the largest per-channel range of the selected samples).  params: MedianParams (median_params()) or its keyword fields (ramp,
        depth)."""
        p = _resolve(params, median_params, kw)
        return self._render_host(self.L.mi355_mosaic_median, imgs, h9s, (C.byref(p),), extra=(want_spread, np.uint8))

    def MosaicMedianDev(self, d_imgs, w, h, ws, h9s, d_canvas, cw, ch, cws, row0=0, rows=-1, d_spread=0, d_count=0, params=None, **kw):
        """mi355_mosaic_median_dev: device frames (0 / None: withheld; d_imgs None when d_canvas and d_spread are 0) into the device canvas and /
        or the maps d_spread (uint8 [ch, cw]) and d_count (uint16 [ch, cw]) (0: not wanted), rows [row0, row0 + rows); complete on return"""
        p = _resolve(params, median_params, kw)
        self._render_dev(self.L.mi355_mosaic_median_dev, d_imgs, w, h, ws, h9s, (C.byref(p),), d_canvas, cw, ch, cws, maps=(d_spread, d_count),
                         stripe=(row0, rows))

    def MosaicMedianInto(self, imgs, img_ids, h9s, out=None, pitch=None, geom=None, params=None, **kw):
        """mi355_mosaic_median_into, sources and destination as MosaicImagesRefinedInto.  Returns (out, cw, ch)."""
        p = _resolve(params, median_params, kw)
        return self._render_into(self.L.mi355_mosaic_median_into, imgs, img_ids, h9s, (C.byref(p),), mosaic_layout, out, pitch, geom)

    def MedianCover(self, w, h, h9s, row0=0, rows=-1, params=None, **kw):
        """mi355_mosaic_median_cover: need[k] = 1 exactly for the frames that are among the selected of at least one pixel of canvas rows
        [row0, row0 + rows)"""
        p = _resolve(params, median_params, kw)
        return self._render_cover(self.L.mi355_mosaic_median_cover, w, h, h9s, (C.byref(p),), row0, rows)

    # ---- lens undistortion (mi355_undistort_*, csrc/undistort.hip) ---------------------------------------------------------
    def UndistortFramesDev(self, d_src, d_dst, w, h, ws_src, ws_dst, cam, params=None, **kw):
        """mi355_undistort_frames_dev: device frames d_src resampled from the distorted camera `cam` (Camera) to the pinhole camera of params
        (UndistortParams / undistort_params() keyword fields) into d_dst (d_dst[k] == d_src[k] with equal pitches: in place).  Complete on
        return; returns n_outside, int64 [n]: the pixels of each frame without a sample."""
        n, sp, w, h, ws_src, _ = _dev_frames(d_src, w, h, ws_src)
        if len(d_dst) != n:
            raise ValueError("d_src and d_dst must list the same frames")
        dp = _dptrs(d_dst, n)
        ws_dst = np.ascontiguousarray(ws_dst, np.int32)
        p = _resolve(params, undistort_params, kw)
        out = np.zeros(n, np.int64)
        self._chk(self.L.mi355_undistort_frames_dev(self._h, sp, dp, _p(w), _p(h), _p(ws_src), _p(ws_dst), n, C.byref(cam), C.byref(p), _p(out)))
        return out

    def UndistortImage(self, img, cam, params=None, out=None, **kw):
        """mi355_undistort_image: a host BGR image [h, w, 3] uint8 resampled; out: the array to write (img itself is allowed), default a new
        one.  Returns (out, n_outside)."""
        if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3 or img.strides[1:] != (3, 1):
            raise ValueError("img must be [h, w, 3] uint8 with contiguous rows")
        out = np.empty_like(img) if out is None else out
        if out.dtype != np.uint8 or out.shape != img.shape or out.strides[1:] != (3, 1):
            raise ValueError("out must have img's shape and contiguous rows")
        h, w = img.shape[:2]
        p = _resolve(params, undistort_params, kw)
        cnt = C.c_int64(0)
        self._chk(self.L.mi355_undistort_image(self._h, C.c_void_p(img.ctypes.data), w, h, int(img.strides[0]), C.c_void_p(out.ctypes.data),
                                               int(out.strides[0]), C.byref(cam), C.byref(p), C.byref(cnt)))
        return out, int(cnt.value)

    # ---- local registration (mi355_tie_residual_stats_*, mi355_solve_local_warps, mi355_apply_local_warps_dev, csrc/local_warp.hip) ------
    def TieResidualStatsDev(self, d_results, n_pairs, w, h, h9s, d_stats, params=None, **kw):
        """mi355_tie_residual_stats_dev: the residual sums of n_pairs device pair records into the device buffer d_stats
        (local_warp_stats_len(n, grid_x, grid_y) int64 values, cleared by the call).  w, h, h9s: the frames' sizes and frame-to-canvas
        matrices.  params: LocalWarpParams (local_warp_params()) or its keyword fields.  Enqueued on the ctx stream."""
        w, h = np.ascontiguousarray(w, np.int32), np.ascontiguousarray(h, np.int32)
        h9s = _h9rows(h9s)
        if not (len(w) == len(h) == len(h9s)):
            raise ValueError("w, h and h9s must list the same frames")
        p = _resolve(params, local_warp_params, kw)
        self._chk(self.L.mi355_tie_residual_stats_dev(self._h, _dptr(d_results), int(n_pairs), _p(w), _p(h), _p(h9s), len(w), C.byref(p),
                                                      _dptr(d_stats)))

    def ApplyLocalWarpsDev(self, d_src, d_dst, w, h, ws_src, ws_dst, grids):
        """mi355_apply_local_warps_dev: device frames d_src resampled by their displacement grids (float32 [n, grid_y + 1, grid_x + 1, 2],
        source pixels) into d_dst (d_dst[k] == d_src[k] with equal pitches: in place).  Complete on return; returns n_clamped, int64 [n]:
        the pixels of each frame whose sample position was clamped to the frame."""
        n, sp, w, h, ws_src, _ = _dev_frames(d_src, w, h, ws_src)
        if len(d_dst) != n:
            raise ValueError("d_src and d_dst must list the same frames")
        dp = _dptrs(d_dst, n)
        ws_dst = np.ascontiguousarray(ws_dst, np.int32)
        g = np.ascontiguousarray(grids, np.float32)
        if g.ndim != 4 or g.shape[0] != n or g.shape[3] != 2:
            raise ValueError("grids must be [n, grid_y + 1, grid_x + 1, 2]")
        out = np.zeros(n, np.int64)
        self._chk(self.L.mi355_apply_local_warps_dev(self._h, sp, dp, _p(w), _p(h), _p(ws_src), _p(ws_dst), n, int(g.shape[2]) - 1, int(g.shape[1]) - 1, _p(g),
                                                     _p(out)))
        return out

    def LocalRegisterDev(self, d_results, n_pairs, d_imgs, w, h, ws, h9s, params=None, **kw):
        """mi355_local_register_dev: residual statistics of the device pair records, the per-frame solve and the apply in place on the
        device frames.  Returns (grids float32 [n, grid_y + 1, grid_x + 1, 2], report LOCAL_WARP_REPORT [n])."""
        n, ptrs, w, h, ws, _ = _dev_frames(d_imgs, w, h, ws)
        h9s = _h9rows(h9s)
        if len(h9s) != n:
            raise ValueError("h9s must list the same frames")
        p = _resolve(params, local_warp_params, kw)
        ok = 1 <= p.grid_x <= 16 and 1 <= p.grid_y <= 16
        grids = np.zeros((n, p.grid_y + 1, p.grid_x + 1, 2) if ok else (n, 1, 1, 2), np.float32)
        rep = np.zeros(n, LOCAL_WARP_REPORT)
        self._chk(self.L.mi355_local_register_dev(self._h, _dptr(d_results), int(n_pairs), ptrs, _p(w), _p(h), _p(ws), n, _p(h9s),
                                                  C.byref(p), _p(grids), _p(rep)))
        return grids, rep

    # ---- pair verification (mi355_pair_edges_dev, mi355_pair_cycles_dev, mi355_pair_residuals_dev, mi355_verify_pairs_dev; csrc/verify.hip) ------
    def PairEdgesDev(self, d_results, n, n_images, d_out):
        """mi355_pair_edges_dev: one PAIR_EDGE per device pair record, device to device (ctx stream)"""
        self._chk(self.L.mi355_pair_edges_dev(self._h, _dptr(d_results), int(n), int(n_images), _dptr(d_out)))

    def PairCyclesDev(self, edges, n_images, cycle_tol=6.0):
        """mi355_pair_cycles_dev: the triangle counts of host PAIR_EDGE records, formed on the device; returns PAIR_CYCLE [n]"""
        e = np.ascontiguousarray(edges, PAIR_EDGE)
        out = np.zeros(len(e), PAIR_CYCLE)
        self._chk(self.L.mi355_pair_cycles_dev(self._h, _p(e), len(e), int(n_images), C.c_double(cycle_tol), _p(out)))
        return out

    def PairResidualsDev(self, d_results, n, h9s, label, d_out):
        """mi355_pair_residuals_dev: one PAIR_RESIDUAL per device pair record under the transforms h9s (float32 [n_images, 9], host) and the
        labels (int32 [n_images], host, or None), device to device (ctx stream)"""
        h9s = _h9rows(h9s)
        lb = _arr(label, np.int32)
        assert lb is None or len(lb) == len(h9s)
        self._chk(self.L.mi355_pair_residuals_dev(self._h, _dptr(d_results), int(n), _p(h9s), _p(lb), len(h9s),
                                                  _dptr(d_out)))

    def VerifyPairsDev(self, d_results, n_pairs, n_images, d_out, fixed=None, params=None, **kw):
        """mi355_verify_pairs_dev: n_pairs device pair records d_results -> d_out (may be d_results) with every usable pair that is not kept
        demoted.  Returns (label int32 [n_images], transforms IMAGE_TRANSFORM [n_images], report VERIFY_REPORT [n_pairs], summary
        VERIFY_SUMMARY scalar).  params: VerifyParams (verify_params()) or its keyword fields."""
        p = _resolve(params, verify_params, kw)
        ff = _arr(fixed, np.int32)
        assert ff is None or len(ff) == int(n_images)
        m = max(int(n_images), 1)
        label, tr = np.zeros(m, np.int32), np.zeros(m, IMAGE_TRANSFORM)
        rep, summ = np.zeros(max(int(n_pairs), 0), VERIFY_REPORT), np.zeros(1, VERIFY_SUMMARY)
        self._chk(self.L.mi355_verify_pairs_dev(self._h, _dptr(d_results), int(n_pairs), int(n_images), _p(ff), C.byref(p),
                                                _dptr(d_out), _p(label), _p(tr), _p(rep), _p(summ)))
        return label, tr, rep, summ[0]

    # ---- guided matching (mi355_guided_select_dev, mi355_guided_match_dev, mi355_guided_match; csrc/guided.hip) ------
    @staticmethod
    def _guided_args(pairs, guides, params, kw):
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        guides = np.ascontiguousarray(guides, np.float32).reshape(-1, 9)
        assert len(pairs) == len(guides)
        return pairs, guides, _resolve(params, default_guided_params, kw)

    def GuidedSelectDev(self, pairs, guides, d_a, d_b, d_nsel, d_dist=0, params=None, **kw):
        """mi355_guided_select_dev: the guided selection of the pairs (int32 [n, 2], host) under the guides (float32 [n, 9], image j -> image i, host)
        into device lists d_a, d_b (n x 400 SFPOINT), d_nsel (n int32) and d_dist (n x 400 int32, or 0); one launch on the ctx stream.
        params: GuidedParams (default_guided_params()) or its keyword fields."""
        pairs, guides, p = self._guided_args(pairs, guides, params, kw)
        self._chk(self.L.mi355_guided_select_dev(self._h, _p(pairs), len(pairs), _p(guides), C.byref(p), _dptr(d_a),
                                                 _dptr(d_b), _dptr(d_nsel), _dptr(d_dist)))

    def GuidedMatchDev(self, pairs, guides, d_out, ransac_dist=2.5, seed=1, params=None, **kw):
        """mi355_guided_match_dev: guided selection plus the pair stage's tail, n PAIR_RESULT records at the device pointer d_out"""
        pairs, guides, p = self._guided_args(pairs, guides, params, kw)
        self._chk(self.L.mi355_guided_match_dev(self._h, _p(pairs), len(pairs), _p(guides), C.byref(p), C.c_float(ransac_dist), C.c_uint32(seed),
                                                _dptr(d_out)))

    def GuidedMatch(self, pairs, guides, ransac_dist=2.5, seed=1, params=None, **kw):
        """mi355_guided_match: the same, returns PAIR_RESULT [n]"""
        pairs, guides, p = self._guided_args(pairs, guides, params, kw)
        out = np.zeros(len(pairs), PAIR_RESULT)
        self._chk(self.L.mi355_guided_match(self._h, _p(pairs), len(pairs), _p(guides), C.byref(p), C.c_float(ransac_dist), C.c_uint32(seed), _p(out)))
        return out

    # ---- overview levels and the striped preview (mi355_mosaic_overview*, mi355_mosaic_preview_into, csrc/overview.hip) ------
    def MosaicOverviewDev(self, d_rows, cw, ch, cws, levels, d_levels, d_covers=None, d_valid_rows=0, nodata=NODATA_NONE, row0=0, rows=-1):
        """mi355_mosaic_overview_dev: d_rows / d_valid_rows are the device addresses of canvas row row0 / map row row0; d_levels[l - 1] the
        whole device buffer of level l (overview_layout), d_covers None or a list whose entries may be 0.  Enqueued on the ctx stream."""
        self._chk(self.L.mi355_mosaic_overview_dev(self._h, _dptr(d_rows), int(cw), int(ch), int(cws),
                                                   _dptr(d_valid_rows), int(nodata), int(levels), _dptrs(d_levels), _dptrs(d_covers),
                                                   int(row0), int(rows)))

    def MosaicOverview(self, canvas, cw, levels, valid=None, nodata=NODATA_NONE, want_covers=False):
        """mi355_mosaic_overview: a host canvas [ch, cws] uint8 (and a [ch, cw] uint16 map for NODATA_MAP) in, the list of level arrays
        [oh_l, ows_l] out -- with want_covers (levels, covers), covers[l - 1] a [oh_l, ow_l] uint16 array."""
        canvas = np.ascontiguousarray(canvas, np.uint8)
        ch, cws = canvas.shape
        v = _arr(valid, np.uint16)
        lv, cv = C.POINTER(C.c_void_p)(), C.POINTER(C.c_void_p)()
        self._chk(self.L.mi355_mosaic_overview(self._h, _p(canvas), int(cw), int(ch), int(cws), _p(v), int(nodata), int(levels), C.byref(lv),
                                               C.byref(cv) if want_covers else None))
        geo = overview_layout(cw, ch, levels)

        outs = [_owned(self.L, C.c_void_p(lv[l]), geo[l][2] * geo[l][1], np.uint8).reshape(geo[l][1], geo[l][2]) for l in range(levels)]
        self.L.mi355_free(lv)
        if not want_covers:
            return outs
        covs = [_owned(self.L, C.c_void_p(cv[l]), geo[l][0] * geo[l][1], np.uint16).reshape(geo[l][1], geo[l][0]) for l in range(levels)]
        self.L.mi355_free(cv)
        return outs, covs

    def MosaicPreviewInto(self, imgs, img_ids, h9s, out=None, pitch=None, geom=None, params=None, want_cover=False, dims=None, **kw):
        """mi355_mosaic_preview_into: level `level` of the named render (render 0 refined, 1 feathered, 2 seamline), sources as
        MosaicImagesRefinedInto.  Returns (out, ow, oh), with want_cover (out, ow, oh, cover [oh, ow] uint16).  dims: (ow, oh) to pass in place
        of the layout's (the library refuses any other)."""
        ptrs, ids, w, h, ws, _keep = self._into_args(imgs, img_ids, geom)
        h9s = _arr(h9s, np.float32)
        p = _resolve(params, preview_params, kw)
        cw, ch, _, _ = mosaic_layout(w, h, h9s)
        ow, oh, _ = overview_layout(cw, ch, p.level)[-1] if 1 <= p.level <= 7 else (cw, ch, 0)      # a bad level is the library's to refuse
        if dims is not None:
            ow, oh = dims
        out, pitch = self._out_array(out, pitch, ow, oh)
        cover = np.zeros((oh, ow), np.uint16) if want_cover else None
        self._chk(self.L.mi355_mosaic_preview_into(self._h, ptrs, _p(ids), _p(w), _p(h), _p(ws), len(ids), _p(h9s), C.byref(p),
                                                   C.c_void_p(out.ctypes.data), int(pitch), _p(cover), int(ow), int(oh)))
        return (out, ow, oh, cover) if want_cover else (out, ow, oh)

    # ---- frames kept in HBM after extraction, renders into caller memory -------------------------------------------------
    def DropFrames(self, img_id=-1):
        """releases the kept frame of img_id (set_option("keep_frames", 1)); img_id < 0: all of them"""
        self._chk(self.L.mi355_drop_frames(self._h, int(img_id)))

    def FrameDev(self, img_id):
        """(device address, w, h, ws) of the kept frame of img_id"""
        d = C.c_void_p()
        w, h, ws = C.c_int(), C.c_int(), C.c_int()
        self._chk(self.L.mi355_get_frame_dev(self._h, int(img_id), C.byref(d), C.byref(w), C.byref(h), C.byref(ws)))
        return d.value or 0, w.value, h.value, ws.value

    def _into_args(self, imgs, img_ids, geom):
        """host pointers (None where a kept frame is the source), ids (-1: the host image) and w, h, ws; geom[k] = (w, h, ws) of an image
        given only by its id (default: the kept frame's)"""
        n = len(imgs) if imgs is not None else len(img_ids)
        ids = np.full(n, -1, np.int32) if img_ids is None else np.ascontiguousarray(img_ids, np.int32)
        keepalive, ptrs = [], (C.c_void_p * n)()
        w, h, ws = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        for k in range(n):
            im = None if imgs is None else imgs[k]
            if im is not None:
                a = np.ascontiguousarray(im, np.uint8)
                keepalive.append(a)
                ptrs[k] = a.ctypes.data
                w[k], h[k], ws[k] = a.shape[1], a.shape[0], a.strides[0]
            elif geom is not None and geom[k] is not None:
                w[k], h[k], ws[k] = geom[k]
            elif ids[k] >= 0:
                _, w[k], h[k], ws[k] = self.FrameDev(int(ids[k]))
        return ptrs, ids, w, h, ws, keepalive

    @staticmethod
    def _out_array(out, pitch, cw, ch):
        if out is None:
            pitch = pitch or (3 * cw + 3) & ~3
            out = np.zeros((ch, pitch), np.uint8)
        if out.dtype != np.uint8 or not out.flags["C_CONTIGUOUS"] or out.ndim < 2:
            raise ValueError("out must be a C-contiguous uint8 array of rows")
        pitch = int(pitch or out.strides[0])
        if ch > 0 and pitch >= 3 * cw and out.nbytes < pitch * (ch - 1) + 3 * cw:
            raise ValueError("out holds %d bytes, the canvas needs %d rows of pitch %d" % (out.nbytes, ch, pitch))
        return out, pitch

    def MosaicImagesRefinedInto(self, imgs, img_ids, h9s, out=None, pitch=None, geom=None):
        """mi355_mosaic_refined_into: image k from the kept frame of img_ids[k] (>= 0) or the host image imgs[k]; the canvas is written into
        out (rows of `pitch` bytes, default out's row stride; out=None: a fresh (ch, cws) array).  Returns (out, cw, ch)."""
        return self._render_into(self.L.mi355_mosaic_refined_into, imgs, img_ids, h9s, (), mosaic_layout, out, pitch, geom)

    def MosaicBlendedInto(self, imgs, img_ids, h9s, keep=None, band=5, out=None, pitch=None, geom=None):
        """mi355_mosaic_blended_into, sources and destination as MosaicImagesRefinedInto.  Returns (out, cw, ch)."""
        keep_a = _arr(keep, np.uint8)
        return self._render_into(self.L.mi355_mosaic_blended_into, imgs, img_ids, h9s, (_p(keep_a), int(band)),
                                 lambda w, h, h9s: blend_layout(w, h, h9s, keep_a), out, pitch, geom)


# ---- host-only helpers (no ctx) ---------------------------------------------------------------------------
def comm_unique_id():
    """128-byte RCCL id for mi355_comm_init (rank 0 creates it, every rank receives it by any transport)"""
    buf = (C.c_uint8 * 128)()
    _host_chk(load_library().mi355_comm_unique_id(buf), "comm_unique_id: librccl not usable")
    return bytes(buf)


def blend_layout(w, h, h9s, keep=None):
    """canvas size (cw, ch, cws) of LaplacianPyramidBlending for these transforms (MosaicImage.cpp:2233-2292)"""
    n, w, h, h9s = _geom(w, h, h9s)
    keep_a = _arr(keep, np.uint8)
    cw, ch, cws = C.c_int(), C.c_int(), C.c_int()
    _host_chk(load_library().mi355_blend_layout(_p(w), _p(h), n, _p(h9s), _p(keep_a), C.byref(cw), C.byref(ch), C.byref(cws)), "blend_layout")
    return cw.value, ch.value, cws.value


def comm_available():
    """True when the library can bind librccl in this process (touches no communicator)"""
    return load_library().mi355_comm_available() == 0


def mosaic_layout(w, h, h9s):
    n, w, h, h9s = _geom(w, h, h9s)
    cw, ch, cws = C.c_int(), C.c_int(), C.c_int()
    dG = np.zeros(2, np.float32)
    _host_chk(load_library().mi355_mosaic_layout(_p(w), _p(h), n, _p(h9s), C.byref(cw), C.byref(ch), C.byref(cws), _p(dG)), "mosaic_layout")
    return cw.value, ch.value, cws.value, dG


def resample_by_overlap(w, h, h9s, overlapT=0.7):
    """ResampleByOverlap (MosaicImage.cpp:2069-2201): keep[k] = vecAbandonInd[k]"""
    n, w, h, h9s = _geom(w, h, h9s)
    keep = np.zeros(n, np.uint8)
    _host_chk(load_library().mi355_resample_by_overlap(_p(w), _p(h), n, _p(h9s), C.c_float(overlapT), _p(keep)), "resample_by_overlap")
    return keep


def surf_pair_schedule(n_images):
    L = load_library()
    n = C.c_int(0)
    L.mi355_surf_pair_schedule(int(n_images), None, 0, C.byref(n))
    out = np.zeros((max(n.value, 1), 2), np.int32)
    L.mi355_surf_pair_schedule(int(n_images), _p(out), n.value, C.byref(n))
    return out[:n.value]


def screen_params(window=0, top_k=256, partners=None, min_score=None, ratio_pct=80):
    """mi355_screen_params: the library's defaults (mi355_default_screen_params) with the given fields replaced"""
    return _params(ScreenParams, "mi355_default_screen_params",
                   dict(window=window, top_k=top_k, partners=partners, min_score=min_score, ratio_pct=ratio_pct))


def gain_params(sigma_n=None, sigma_g=None, channels=None, step=None):
    """mi355_gain_params: the library's defaults (mi355_default_gain_params: 10, 0.1, 3, 8) with the given fields replaced"""
    return _params(GainParams, "mi355_default_gain_params", dict(sigma_n=sigma_n, sigma_g=sigma_g, channels=channels, step=step))


def block_gain_params(sigma_n=None, sigma_g=None, channels=None, step=None, grid_x=None, grid_y=None, smooth=None):
    """mi355_block_gain_params: the library's defaults (mi355_default_block_gain_params: 10, 0.1, 3, 8, 8 x 6, 2) with the given fields replaced"""
    return _params(BlockGainParams, "mi355_default_block_gain_params",
                   dict(sigma_n=sigma_n, sigma_g=sigma_g, channels=channels, step=step, grid_x=grid_x, grid_y=grid_y, smooth=smooth))


def sharp_params(prior=None, blur_ratio=None, step=None):
    """mi355_sharp_params: the library's defaults (mi355_default_sharp_params: 0.01, 0.58, 8) with the given fields replaced"""
    return _params(SharpParams, "mi355_default_sharp_params", dict(prior=prior, blur_ratio=blur_ratio, step=step))


def cover_params(step=None, min_depth=None, max_loss=None):
    """mi355_cover_params: the library's defaults (mi355_default_cover_params: 8, 1, 0) with the given fields replaced"""
    return _params(CoverParams, "mi355_default_cover_params", dict(step=step, min_depth=min_depth, max_loss=max_loss))


def _cover_args(w, h, h9s, keep):
    n, w, h, h9s = _geom(w, h, h9s)
    if keep is not None:
        keep = np.ascontiguousarray(keep, np.uint8)
        if len(keep) != n:
            raise ValueError("keep holds %d bytes for %d frames" % (len(keep), n))
    return w, h, h9s, n, keep


def _cover_lists(order, pairs):
    if order is not None:
        order = np.ascontiguousarray(np.asarray(order, np.int32).reshape(-1))
    ab = np.ascontiguousarray(np.asarray(pairs if pairs is not None else [], np.int32).reshape(-1, 2))
    return order, (len(order) if order is not None else 0), ab, len(ab)


def cover_select(w, h, h9s, stats_fn, order=None, pairs=None, keep=None, params=None, **kw):
    """mi355_cover_select (host only, no device): the selection of "cover depth" with the statistics of every round supplied by
    stats_fn(keep [n] uint8) -> COVER_FRAME_STATS [n] (or an [n, 8] integer array).  Returns (status [n] uint8, keep_out [n] uint8, rounds,
    lost).  An exception raised by stats_fn ends the selection and is raised again."""
    L = load_library()
    w, h, h9s, n, keep = _cover_args(w, h, h9s, keep)
    order, n_order, ab, npairs = _cover_lists(order, pairs)
    p = _resolve(params, cover_params, kw)
    raised = []

    def call(_user, keep_ptr, fs_ptr):
        try:
            kp = np.ctypeslib.as_array(C.cast(keep_ptr, C.POINTER(C.c_uint8)), (n,)).copy()
            fs = np.asarray(stats_fn(kp))
            fs = np.ascontiguousarray(fs["at_depth"] if fs.dtype.names else fs, np.int64).reshape(n, 8)
            C.memmove(fs_ptr, fs.ctypes.data, 64 * n)
            return 0
        except BaseException as e:                                   # nothing may unwind through the C frames
            raised.append(e)
            return -2                                                # MI355_ERR_FAILED
    cb = COVER_STATS_FN(call)
    status, keep_out = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint8)
    rounds, lost = C.c_int32(0), C.c_int64(0)
    rc = L.mi355_cover_select(_p(w), _p(h), n, _p(h9s), _p(keep), _p(order), n_order, _p(ab), npairs, C.byref(p), cb, None,
                              _p(status), _p(keep_out), C.byref(rounds), C.byref(lost))
    if raised:
        raise raised[0]
    _host_chk(rc, positive=False)
    return status[:n], keep_out[:n], int(rounds.value), int(lost.value)


def feather_params(ramp=None):
    """mi355_feather_params: the library's defaults (mi355_default_feather_params: ramp 0 = a full tent per frame) with the given fields replaced"""
    return _params(FeatherParams, "mi355_default_feather_params", dict(ramp=ramp))


def seamline_params(ramp=None):
    """mi355_seamline_params: the library's defaults (mi355_default_seamline_params: ramp 0 = a full tent per frame) with the given fields replaced"""
    return _params(SeamlineParams, "mi355_default_seamline_params", dict(ramp=ramp))


def median_params(ramp=None, depth=None):
    """mi355_median_params: the library's defaults (mi355_default_median_params: ramp 0 = a full tent per frame, depth 0 = 5 frames) with the
    given fields replaced"""
    return _params(MedianParams, "mi355_default_median_params", dict(ramp=ramp, depth=depth))


def seamcut_params(ramp=None, level=None, depth=None, data_weight=None, diff_weight=None, seam_penalty=None, miss_cost=None):
    """mi355_seamcut_params: the library's defaults (mi355_default_seamcut_params: ramp 0, level 3, depth 4, costs 1, 2, 2, 32) with the given
    fields replaced"""
    return _params(SeamCutParams, "mi355_default_seamcut_params",
                   dict(ramp=ramp, level=level, depth=depth, data_weight=data_weight, diff_weight=diff_weight, seam_penalty=seam_penalty, miss_cost=miss_cost))


def seam_grid(w, h, h9s, level):
    """(gw, gh): the cell grid of the survey's canvas at `level`"""
    cw, ch, _, _ = mosaic_layout(w, h, h9s)
    s = 1 << int(level)
    return (cw + s - 1) // s, (ch + s - 1) // s


def blend_seam_grid(w, h, h9s, level, keep=None):
    """(gw, gh): the cell grid of the blend's canvas (blend_layout) at `level`"""
    cw, ch, _ = blend_layout(w, h, h9s, keep)
    s = 1 << int(level)
    return (cw + s - 1) // s, (ch + s - 1) // s


def _report(r):
    return dict(energy_before=int(r.energy_before), energy_after=int(r.energy_after), changed=int(r.changed), fallback=int(r.fallback))


def seam_labels_host(cand, params=None, **kw):
    """mi355_seam_labels_host: cell records [gh, gw] of SEAM_CELL in, (cells [gh, gw] uint16, report dict) out; no GPU"""
    cand = np.ascontiguousarray(cand, SEAM_CELL)
    gh, gw = cand.shape
    p = _resolve(params, seamcut_params, kw)
    cells = np.zeros((gh, gw), np.uint16)
    r = SeamReport()
    _host_chk(load_library().mi355_seam_labels_host(_p(cand), int(gw), int(gh), C.byref(p), _p(cells), C.byref(r)), "seam_labels_host: bad arguments")
    return cells, _report(r)


def undistort_params(out_fx=None, out_fy=None, out_cx=None, out_cy=None, fill=None):
    """mi355_undistort_params: the library's defaults (mi355_default_undistort_params: the camera's own intrinsics, fill 0) with the given
    fields replaced"""
    return _params(UndistortParams, "mi355_default_undistort_params", dict(out_fx=out_fx, out_fy=out_fy, out_cx=out_cx, out_cy=out_cy, fill=fill))


def tie_params(radius=None, search=None, drop_mask=None, min_ncc=None):
    """mi355_tie_params: the library's defaults (radius 7, search 3, drop_mask 0, min_ncc 0.7) with the given fields replaced"""
    return _params(TieParams, "mi355_default_tie_params", dict(radius=radius, search=search, drop_mask=drop_mask, min_ncc=min_ncc))


def local_warp_params(grid_x=None, grid_y=None, min_ties=None, max_residual=None, max_shift=None, smooth=None, prior=None):
    """mi355_local_warp_params: the library's defaults (mi355_default_local_warp_params) with the given fields replaced"""
    return _params(LocalWarpParams, "mi355_default_local_warp_params",
                   dict(grid_x=grid_x, grid_y=grid_y, min_ties=min_ties, max_residual=max_residual, max_shift=max_shift, smooth=smooth, prior=prior))


def verify_params(cycle_tol=None, gate_abs=None, gate_k=None, max_rounds=None, bridges=None):
    """mi355_verify_params: the library's defaults (6.0, 3.0, 4.0, 8, 1) with the given fields replaced"""
    return _params(VerifyParams, "mi355_default_verify_params",
                   dict(cycle_tol=cycle_tol, gate_abs=gate_abs, gate_k=gate_k, max_rounds=max_rounds, bridges=bridges))


def default_guided_params(radius=None, max_dist2=None, ratio=None, reserved=None):
    """mi355_guided_params: the library's defaults (radius 4, max_dist2 90000, ratio 0.8) with the given fields replaced"""
    return _params(GuidedParams, "mi355_default_guided_params", dict(radius=radius, max_dist2=max_dist2, ratio=ratio, reserved=reserved))


def guided_candidates(w, h, transforms, have=None, min_points=0, max_pairs=None):
    """mi355_guided_candidates (host only): the pairs (int32 [n, 2], ascending) the alignment `transforms` (float32 [n_images, 9], frame -> canvas,
    m[8] == 0: not placed) says overlap and `have` ([m, 2]) does not cover, with their guides (float32 [n, 9], image j -> image i).
    max_pairs=None sizes the buffers by a count-only call first; an explicit max_pairs below the count raises (the count is in the message)."""
    L = load_library()
    if max_pairs is None:
        max_pairs = guided_candidates_count(w, h, transforms, have, min_points)
    t = np.ascontiguousarray(transforms, np.float32).reshape(-1, 9)
    hv = np.zeros((0, 2), np.int32) if have is None else np.ascontiguousarray(have, np.int32).reshape(-1, 2)
    n = C.c_int(0)
    pairs, guides = np.zeros((max(int(max_pairs), 1), 2), np.int32), np.zeros((max(int(max_pairs), 1), 9), np.float32)
    _host_chk(L.mi355_guided_candidates(int(w), int(h), len(t), _p(t), _p(hv), len(hv), int(min_points), _p(pairs), _p(guides), int(max_pairs), C.byref(n)), positive=False)
    return pairs[:n.value].copy(), guides[:n.value].copy()


def guided_candidates_count(w, h, transforms, have=None, min_points=0):
    """mi355_guided_candidates with pairs_ij == NULL: the number of candidate pairs"""
    L = load_library()
    t = np.ascontiguousarray(transforms, np.float32).reshape(-1, 9)
    hv = np.zeros((0, 2), np.int32) if have is None else np.ascontiguousarray(have, np.int32).reshape(-1, 2)
    n = C.c_int(0)
    _host_chk(L.mi355_guided_candidates(int(w), int(h), len(t), _p(t), _p(hv), len(hv), int(min_points), None, None, 0, C.byref(n)), positive=False)
    return n.value


def merge_pair_results(base, extra):
    """mi355_merge_pair_results (host only): base records keep their places, an extra record of the same (i, j) replaces one with a smaller n_in,
    the others are appended in order; returns PAIR_RESULT [n_out]"""
    L = load_library()
    b = np.ascontiguousarray(base, PAIR_RESULT)
    e = np.ascontiguousarray(extra, PAIR_RESULT)
    out = np.zeros(max(len(b) + len(e), 1), PAIR_RESULT)
    n = C.c_int(0)
    _host_chk(L.mi355_merge_pair_results(_p(b), len(b), _p(e), len(e), _p(out), C.byref(n)), positive=False)
    return out[:n.value].copy()


def pair_edges_host(results, n_images):
    """mi355_pair_edges_host (host only): PAIR_EDGE [n] of host PAIR_RESULT records"""
    L = load_library()
    r = np.ascontiguousarray(results, PAIR_RESULT)
    out = np.zeros(len(r), PAIR_EDGE)
    _host_chk(L.mi355_pair_edges_host(_p(r), len(r), int(n_images), _p(out)), positive=False)
    return out


def pair_cycles_host(edges, n_images, cycle_tol=6.0):
    """mi355_pair_cycles_host (host only): PAIR_CYCLE [n] of PAIR_EDGE records"""
    L = load_library()
    e = np.ascontiguousarray(edges, PAIR_EDGE)
    out = np.zeros(len(e), PAIR_CYCLE)
    _host_chk(L.mi355_pair_cycles_host(_p(e), len(e), int(n_images), C.c_double(cycle_tol), _p(out)), positive=False)
    return out


def pair_residuals_host(results, h9s, label=None):
    """mi355_pair_residuals_host (host only): PAIR_RESIDUAL [n] of host PAIR_RESULT records under h9s (float32 [n_images, 9]) and label"""
    L = load_library()
    r = np.ascontiguousarray(results, PAIR_RESULT)
    h9s = _h9rows(h9s)
    lb = _arr(label, np.int32)
    assert lb is None or len(lb) == len(h9s)
    out = np.zeros(len(r), PAIR_RESIDUAL)
    _host_chk(L.mi355_pair_residuals_host(_p(r), len(r), _p(h9s), _p(lb), len(h9s), _p(out)), positive=False)
    return out


def verify_pairs_results(results, n_images, fixed=None, params=None, **kw):
    """mi355_verify_pairs_results (host only): -> (records with the pairs that are not kept demoted, label int32 [n_images], transforms
    IMAGE_TRANSFORM [n_images], report VERIFY_REPORT [n], summary VERIFY_SUMMARY scalar)"""
    L = load_library()
    r = np.ascontiguousarray(results, PAIR_RESULT)
    p = _resolve(params, verify_params, kw)
    ff = _arr(fixed, np.int32)
    assert ff is None or len(ff) == int(n_images)
    m = max(int(n_images), 1)
    out, label, tr = np.zeros(len(r), PAIR_RESULT), np.zeros(m, np.int32), np.zeros(m, IMAGE_TRANSFORM)
    rep, summ = np.zeros(len(r), VERIFY_REPORT), np.zeros(1, VERIFY_SUMMARY)
    _host_chk(L.mi355_verify_pairs_results(_p(r), len(r), int(n_images), _p(ff), C.byref(p), _p(out), _p(label), _p(tr), _p(rep), _p(summ)), positive=False)
    return out, label, tr, rep, summ[0]


def local_warp_stats_len(n, grid_x, grid_y):
    """int64 values of the statistics of n frames: MI355_LOCAL_WARP_STATS_STRIDE per frame and a tail of 8"""
    return int(n) * (7 * (int(grid_x) + 1) * (int(grid_y) + 1) + 8) + 8


def tie_residual_stats_host(results, w, h, h9s, params=None, **kw):
    """mi355_tie_residual_stats_host (host only): the residual sums of host PAIR_RESULT records, int64 [local_warp_stats_len(...)]"""
    L = load_library()
    res = np.ascontiguousarray(results, PAIR_RESULT)
    w, h = np.ascontiguousarray(w, np.int32), np.ascontiguousarray(h, np.int32)
    h9s = _h9rows(h9s)
    if not (len(w) == len(h) == len(h9s)):
        raise ValueError("w, h and h9s must list the same frames")
    p = _resolve(params, local_warp_params, kw)
    ok = 1 <= p.grid_x <= 16 and 1 <= p.grid_y <= 16
    st = np.zeros(local_warp_stats_len(len(w), p.grid_x, p.grid_y) if ok else 8, np.int64)
    _host_chk(L.mi355_tie_residual_stats_host(_p(res), len(res), _p(w), _p(h), _p(h9s), len(w), C.byref(p), _p(st)), positive=False)
    return st


def solve_local_warps(stats, n, params=None, **kw):
    """mi355_solve_local_warps (host only): (grids float32 [n, grid_y + 1, grid_x + 1, 2], report LOCAL_WARP_REPORT [n]) from the sums"""
    L = load_library()
    p = _resolve(params, local_warp_params, kw)
    ok = 1 <= p.grid_x <= 16 and 1 <= p.grid_y <= 16
    st = np.ascontiguousarray(stats, np.int64)
    if ok and st.size != local_warp_stats_len(n, p.grid_x, p.grid_y):
        raise ValueError("stats must hold local_warp_stats_len(n, grid_x, grid_y) values")
    grids = np.zeros((n, p.grid_y + 1, p.grid_x + 1, 2) if ok else (n, 1, 1, 2), np.float32)
    rep = np.zeros(n, LOCAL_WARP_REPORT)
    _host_chk(L.mi355_solve_local_warps(_p(st), int(n), C.byref(p), _p(grids), _p(rep)), positive=False)
    return grids, rep


def undistort_fit(cam, w, h):
    """mi355_undistort_fit (host only): the UndistortParams of the widest pinhole camera whose w x h border lies inside the source"""
    L = load_library()
    p = UndistortParams()
    _host_chk(L.mi355_undistort_fit(_ref(cam), int(w), int(h), C.byref(p)), positive=False)
    return p


def undistort_map(cam, w, h, params=None, **kw):
    """mi355_undistort_map (host only): (xs, ys), float32 [h, w] each: the source coordinate of every output pixel"""
    L = load_library()
    p = _resolve(params, undistort_params, kw)
    ok = 0 < int(w) <= 1 << 20 and 0 < int(h) <= 1 << 20
    xs, ys = (np.zeros((int(h), int(w)) if ok else (1, 1), np.float32) for _ in range(2))
    _host_chk(L.mi355_undistort_map(_ref(cam), C.byref(p), int(w), int(h), _p(xs), _p(ys)), positive=False)
    return xs, ys


def preview_params(render=None, ramp=None, level=None, nodata=None):
    """mi355_preview_params: the library's defaults (refined render, ramp 0, level 3, exact coverage) with the given fields replaced"""
    return _params(PreviewParams, "mi355_default_preview_params", dict(render=render, ramp=ramp, level=level, nodata=nodata))


def overview_layout(cw, ch, levels):
    """mi355_overview_layout: [(ow_l, oh_l, ows_l) for l = 1 .. levels]"""
    n = max(int(levels), 0)
    ow, oh, ows = np.zeros(n + 1, np.int32), np.zeros(n + 1, np.int32), np.zeros(n + 1, np.int32)
    L = load_library()
    rc = L.mi355_overview_layout(int(cw), int(ch), int(levels), _p(ow), _p(oh), _p(ows))
    if rc != 0:
        raise Mi355Error(rc, (L.mi355_last_error(None) or b"overview_layout").decode())
    return [(int(ow[l]), int(oh[l]), int(ows[l])) for l in range(n)]


def solve_gains(pair_stats, frame_cover, params=None, **kw):
    """mi355_solve_gains (host only): gains [n, 3] float32 from GAIN_PAIR_STATS records and the frames' cover counts"""
    L = load_library()
    st = np.ascontiguousarray(pair_stats, GAIN_PAIR_STATS)
    cover = np.ascontiguousarray(frame_cover, np.int64)
    n = len(cover)
    p = _resolve(params, gain_params, kw)
    g = np.zeros((max(n, 0), 3), np.float32)
    _host_chk(L.mi355_solve_gains(_p(st), len(st), _p(cover), n, C.byref(p), _p(g)), positive=False)
    return g


def solve_sharpness(pair_stats, n, params=None, **kw):
    """mi355_solve_sharpness (host only): (sharp [n] float32, rel [n] float64) from SHARP_PAIR_STATS records"""
    L = load_library()
    st = np.ascontiguousarray(pair_stats, SHARP_PAIR_STATS)
    n = int(n)
    p = _resolve(params, sharp_params, kw)
    sharp, rel = np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.float64)
    _host_chk(L.mi355_solve_sharpness(_p(st), len(st), n, C.byref(p), _p(sharp), _p(rel)), positive=False)
    return sharp[:max(n, 0)], rel[:max(n, 0)]


def select_sharp_frames(pair_stats, n, params=None, **kw):
    """mi355_select_sharp_frames (host only): (status [n] uint8 -- 0 kept, 1 blurred and dropped, 2 blurred but kept (a cut vertex), 3 no
    usable pair --, sharp [n] float32) from SHARP_PAIR_STATS records"""
    L = load_library()
    st = np.ascontiguousarray(pair_stats, SHARP_PAIR_STATS)
    n = int(n)
    p = _resolve(params, sharp_params, kw)
    status, sharp = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.float32)
    _host_chk(L.mi355_select_sharp_frames(_p(st), len(st), n, C.byref(p), _p(status), _p(sharp)), positive=False)
    return status[:max(n, 0)], sharp[:max(n, 0)]


def drop_sharp_frames(h9s, status):
    """h9s [n, 9] float32 with m8 = 0 (the renders' skip convention) for the frames a sharpness selection dropped (status 1)"""
    out = np.array(h9s, np.float32).reshape(-1, 9).copy()
    out[np.asarray(status) == SHARP_DROPPED, 8] = 0
    return out


def solve_block_gains(records, pairs, cell_cover, params=None, **kw):
    """mi355_solve_block_gains (host only): smoothed gain maps [n, grid_y, grid_x, 3] float32 from BLOCK_GAIN_STATS records, the pair list
    they index and the cell cover [n, grid_y * grid_x]"""
    L = load_library()
    st = np.ascontiguousarray(records, BLOCK_GAIN_STATS)
    ab = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
    cover = np.ascontiguousarray(cell_cover, np.int64)
    n = len(cover)
    p = _resolve(params, block_gain_params, kw)
    gx, gy = p.grid_x, p.grid_y
    ok = 1 <= gx <= 16 and 1 <= gy <= 16
    if ok and cover.size != n * gx * gy:
        raise ValueError("cell_cover must hold n x grid_y * grid_x values")
    g = np.zeros((n, gy, gx, 3) if ok else (n, 1, 1, 3), np.float32)
    _host_chk(L.mi355_solve_block_gains(_p(st), C.c_int64(len(st)), _p(ab), len(ab), _p(cover), n, C.byref(p), _p(g)), positive=False)
    return g


def pair_schedule(n_images, window, rank=0, world=1):
    L = load_library()
    n = C.c_int(0)
    L.mi355_pair_schedule(int(n_images), int(window), int(rank), int(world), None, 0, C.byref(n))
    out = np.zeros((max(n.value, 1), 2), np.int32)
    _host_chk(L.mi355_pair_schedule(int(n_images), int(window), int(rank), int(world), _p(out), n.value, C.byref(n)), "pair_schedule")
    return out[:n.value]


def write_match_pairs(path, v):
    v = np.ascontiguousarray(v, MATCHPAIR)
    _write("mi355_write_match_pairs", "write_match_pairs", path, v, len(v))


def load_match_pairs(path):
    return _load("mi355_load_match_pairs", "load_match_pairs", MATCHPAIR, path.encode())


def write_match_pairs_txt(path, v):
    v = np.ascontiguousarray(v, MATCHPAIR)
    _write("mi355_write_match_pairs_txt", "write_match_pairs_txt", path, v, len(v))


def write_transforms(path, t):
    t = np.ascontiguousarray(t, IMAGE_TRANSFORM)
    _write("mi355_write_transforms", "write_transforms", path, t, len(t))


def load_transforms(path, tran0=False):
    """ImportTransform's format (count + 9 floats each), or with tran0=True the rows OutTransform writes (tran0.txt)"""
    return _load("mi355_load_tran0" if tran0 else "mi355_load_transforms", "load_transforms", IMAGE_TRANSFORM, path.encode())


def write_keypoints(path, kp):
    kp = np.ascontiguousarray(kp, KEYPOINT)
    _write("mi355_write_keypoints", "write_keypoints", path, kp, len(kp))


def load_keypoints(path):
    return _load("mi355_load_keypoints", "load_keypoints", KEYPOINT, path.encode())


def write_descriptors_xml(path, desc):
    """discriptor_%d.xml (cv::FileStorage << "descriptor" << Mat CV_32F), OpenCV 2.4's XML layout (unpinned: the reference commits no such file)"""
    d = np.ascontiguousarray(desc, np.float32)
    if d.ndim != 2:
        raise ValueError("descriptors: a 2-D array")
    _write("mi355_write_descriptors_xml", "write_descriptors_xml", path, d, int(d.shape[0]), int(d.shape[1]))


def load_descriptors_xml(path):
    L = load_library()
    ptr, r, c = C.c_void_p(), C.c_int(0), C.c_int(0)
    _host_chk(L.mi355_load_descriptors_xml(path.encode(), C.byref(ptr), C.byref(r), C.byref(c)), "load_descriptors_xml")
    return _owned(L, ptr, r.value * c.value, np.float32).reshape(r.value, c.value)


def results_to_match_pairs(results, fixed_flags=None):
    results = np.ascontiguousarray(results, PAIR_RESULT)
    ff = _arr(fixed_flags, np.int32)
    return _load("mi355_results_to_match_pairs", "results_to_match_pairs", MATCHPAIR, _p(results), len(results), _p(ff))


def global_affine_align(match_pairs, n_images, fixed=None):
    v = np.ascontiguousarray(match_pairs, MATCHPAIR)
    ff = _arr(fixed, np.int32)
    out = np.zeros(n_images, IMAGE_TRANSFORM)
    _host_chk(load_library().mi355_global_affine_align(_p(v), len(v), int(n_images), _p(ff), _p(out)), "global_affine_align")
    return out


def select_connected_results(results, n_images):
    """Select_Connected_Matched_Images straight from PAIR_RESULT records (accepted pairs with inliers are the edges)"""
    r = np.ascontiguousarray(results, PAIR_RESULT)
    label = np.zeros(n_images, np.int32)
    _host_chk(load_library().mi355_select_connected_results(_p(r), len(r), int(n_images), _p(label)), "select_connected_results")
    return label


def global_affine_align_results(results, n_images, fixed=None, label=None):
    """global_affine_align straight from PAIR_RESULT records; label: use only the pairs whose two images are labelled"""
    r = np.ascontiguousarray(results, PAIR_RESULT)
    ff = _arr(fixed, np.int32)
    lb = _arr(label, np.int32)
    out = np.zeros(n_images, IMAGE_TRANSFORM)
    _host_chk(load_library().mi355_global_affine_align_results(_p(r), len(r), int(n_images), _p(ff), _p(lb), _p(out)), "global_affine_align_results")
    return out


def pair_moments_host(results):
    """the second moments of every record's inlier coordinates, summed on the host (what mi355_pair_moments_dev forms on the device)"""
    r = np.ascontiguousarray(results, PAIR_RESULT)
    out = np.zeros(len(r), PAIR_MOMENTS)
    _host_chk(load_library().mi355_pair_moments_host(_p(r), len(r), _p(out)), "pair_moments_host")
    return out


def projective_params(**kw):
    """mi355_default_projective_params, with fields overridden by keyword"""
    return _params(ProjectiveParams, "mi355_default_projective_params", kw)


def _projective_args(w, h, start, fixed, label):
    st = np.ascontiguousarray(start, IMAGE_TRANSFORM)
    i32 = lambda a: _arr(a, np.int32)
    w, h, fixed, label = i32(w), i32(h), i32(fixed), i32(label)
    for a in (w, h, fixed, label):
        assert a is None or len(a) == len(st)
    return w, h, st, fixed, label


def pair_normal_blocks_host(results, h8, part):
    """the normal-equation block of every record at the parameters h8 (n_images x 8) and flags part, on the host (what
    mi355_pair_normal_blocks_dev forms on the device)"""
    r = np.ascontiguousarray(results, PAIR_RESULT)
    h8 = np.ascontiguousarray(h8, np.float64).reshape(-1, 8)
    part = np.ascontiguousarray(part, np.uint8)
    assert len(h8) == len(part)
    out = np.zeros(len(r), PAIR_NORMAL_BLOCK)
    L = load_library()
    _host_chk(L.mi355_pair_normal_blocks_host(_p(r), len(r), _p(h8), _p(part), len(part), _p(out)))
    return out


def _projective_host(fn, data, w, h, start, fixed, label, params):
    w, h, st, fixed, label = _projective_args(w, h, start, fixed, label)
    out, rep = np.zeros(len(st), IMAGE_TRANSFORM), ProjectiveReport()
    L = load_library()
    _host_chk(getattr(L, fn)(_p(data), len(data), len(st), _p(w), _p(h), _p(fixed), _p(label), _p(st), _ref(params), _p(out), C.byref(rep)))
    return out, rep.as_dict()


def global_projective_refine_results(results, w, h, start, fixed=None, label=None, params=None):
    """the projective refinement of `start` (IMAGE_TRANSFORM per image, e.g. the affine alignment's) on host PAIR_RESULT records;
    returns (transforms, report dict)"""
    return _projective_host("mi355_global_projective_refine_results", np.ascontiguousarray(results, PAIR_RESULT), w, h, start, fixed, label, params)


def global_projective_refine(match_pairs, w, h, start, fixed=None, label=None, params=None):
    """the same on the flat MATCHPAIR list (a run of equal image indices is one pair)"""
    return _projective_host("mi355_global_projective_refine", np.ascontiguousarray(match_pairs, MATCHPAIR), w, h, start, fixed, label, params)


def calib_params(**kw):
    """mi355_default_calib_params (20 trials, mask k1 | k2, min_ties 16, lambda 1e-3, up and down 10, min_rel_decrease 1e-6), with fields
    overridden by keyword"""
    return _params(CalibParams, "mi355_default_calib_params", kw)


def pair_calib_blocks_host(results, h8, cam, min_ties=16):
    """the calibration's normal-equation block of every record at the camera `cam` and the states h8 (one row of 8 per record), on the host
    (what mi355_pair_calib_blocks_dev forms on the device)"""
    r = np.ascontiguousarray(results, PAIR_RESULT)
    h8 = np.ascontiguousarray(h8, np.float64).reshape(-1, 8)
    assert len(h8) == len(r)
    out = np.zeros(len(r), PAIR_CALIB_BLOCK)
    L = load_library()
    _host_chk(L.mi355_pair_calib_blocks_host(_p(r), len(r), _p(h8), _ref(cam), int(min_ties), _p(out)))
    return out


def _calibrate_host(fn, data, start, params, kw):
    p = _resolve(params, calib_params, kw)
    out, rep = Camera(), CalibReport()
    L = load_library()
    _host_chk(getattr(L, fn)(_p(data), len(data), _ref(start), C.byref(p), C.byref(out), C.byref(rep)))
    return out, rep.as_dict()


def calibrate_lens_results(results, start, params=None, **kw):
    """mi355_calibrate_lens_results: the Brown-Conrady coefficients of the camera `start` (Camera; its intrinsics are held fixed, its
    coefficients are the start) from host PAIR_RESULT records of the original frames; params: CalibParams or its keyword fields.
    Returns (Camera, report dict)"""
    return _calibrate_host("mi355_calibrate_lens_results", np.ascontiguousarray(results, PAIR_RESULT), start, params, kw)


def calibrate_lens(match_pairs, start, params=None, **kw):
    """the same on the flat MATCHPAIR list (a run of equal image indices is one pair; its start homography is fitted to its own ties)"""
    return _calibrate_host("mi355_calibrate_lens", np.ascontiguousarray(match_pairs, MATCHPAIR), start, params, kw)


def match_pairs_to_results(match_pairs):
    """mi355_match_pairs_to_results: the flat MATCHPAIR list as accepted PAIR_RESULT records (runs cut at 400), each with the least-squares
    homography of its own ties as H"""
    v = np.ascontiguousarray(match_pairs, MATCHPAIR)
    L = load_library()
    n = C.c_int(0)
    rc = L.mi355_match_pairs_to_results(_p(v), len(v), None, 0, C.byref(n))
    out = np.zeros(n.value, PAIR_RESULT)
    if rc == 0 and n.value:
        rc = L.mi355_match_pairs_to_results(_p(v), len(v), _p(out), n.value, C.byref(n))
    _host_chk(rc)
    return out


def select_connected_moments(moments, n_images):
    m = np.ascontiguousarray(moments, PAIR_MOMENTS)
    label = np.zeros(n_images, np.int32)
    _host_chk(load_library().mi355_select_connected_moments(_p(m), len(m), int(n_images), _p(label)), "select_connected_moments")
    return label


def global_affine_align_moments(moments, n_images, fixed=None, label=None):
    """the global alignment from the pairs' second moments: the same bits as global_affine_align_results on the records they were formed from"""
    m = np.ascontiguousarray(moments, PAIR_MOMENTS)
    ff = _arr(fixed, np.int32)
    lb = _arr(label, np.int32)
    out = np.zeros(n_images, IMAGE_TRANSFORM)
    _host_chk(load_library().mi355_global_affine_align_moments(_p(m), len(m), int(n_images), _p(ff), _p(lb), _p(out)), "global_affine_align_moments")
    return out


def select_connected(match_pairs, n_images):
    v = np.ascontiguousarray(match_pairs, MATCHPAIR)
    label = np.zeros(n_images, np.int32)
    _host_chk(load_library().mi355_select_connected(_p(v), len(v), int(n_images), _p(label)), "select_connected")
    return label
