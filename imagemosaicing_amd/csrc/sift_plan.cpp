// csrc/sift_plan.cpp -- see sift_plan.h
#include "sift_plan.h"
#include <algorithm>
#include <cmath>

namespace sift_plan {

int gauss_taps(double sigma, float* k) {
    const int ksize = ((int)lrint(sigma * 8.0 + 1.0)) | 1;
    const int r = ksize / 2;
    // cv::getGaussianKernel(ksize, sigma, CV_32F): each exp() rounded to float, the floats summed in double, taps (float)(tap / sum)
    double sum = 0.0;
    const double scale2x = -0.5 / (sigma * sigma);
    for (int i = 0; i < ksize; i++) { const double x = (double)i - (double)(ksize - 1) * 0.5; k[i] = (float)std::exp(scale2x * x * x); sum += (double)k[i]; }
    sum = 1.0 / sum;
    for (int i = 0; i < ksize; i++) k[i] = (float)((double)k[i] * sum);
    return r;
}

const PyramidTaps& pyramid_taps() {
    static const PyramidTaps taps = [] {
        PyramidTaps t = {};
        // double math on the host, like the oracle
        const double sigma = 1.6, k = std::pow(2.0, 1.0 / N_LAYERS);
        for (int i = 1; i < N_LEVELS; i++) {
            const double sp = std::pow(k, (double)(i - 1)) * sigma, st = sp * k;
            t.lv[i].r = gauss_taps(std::sqrt(st * st - sp * sp), t.lv[i].k);
        }
        // base level: createInitialImage(image, false, sigma) blurs with sqrtf(max(sigma^2 - 0.5^2, 0.01f)), computed in float
        const float sd = std::sqrt(std::max((float)sigma * (float)sigma - 0.25f, 0.01f));
        t.base.r = gauss_taps((double)sd, t.base.k);
        return t;
    }();
    return taps;
}

static inline size_t up64(size_t v) { return (v + 63) & ~(size_t)63; }

Layout make_layout(int w, int h, bool keepall, int kmax, std::string& err) {
    Layout l = {};
    l.w = w; l.h = h; l.keepall = keepall; l.kmax = kmax;
    if (w >= (1 << 20) || h >= (1 << 20)) { err = "sift: image too large"; return l; }
    if (w < 16 || h < 16) { err = "sift: image too small"; return l; }      // (16: two octaves, the first of them 16 >= 2 IMG_BORDER + 2 wide)
    const size_t px0 = (size_t)w * h;
    if (4 * px0 + 1024 > 0xfffffff0ull) { err = "sift: image too large"; return l; }      // candidates are counted in 32 bits
    // octave 0 is the image itself (no doubling in the reference's OpenCV build); nOctaves = cvRound(log2(min(w, h)) - 2)
    const int nOct = std::min((int)lrint(std::log((double)std::min(w, h)) / std::log(2.0) - 2.0), MAX_OCT);
    Strides& bs = l.bs;
    for (int o = 0; o < nOct; o++) {
        Octave& oc = l.oc[o];
        oc.w = w >> o; oc.h = h >> o;
        if (oc.w < 2 * IMG_BORDER + 2 || oc.h < 2 * IMG_BORDER + 2) break;          // no keypoint can exist in smaller octaves
        const size_t px = (size_t)oc.w * oc.h;
        for (int i = 0; i < N_LEVELS; i++) { oc.lv[i] = bs.pyr; bs.pyr += up64(px); }      // every level starts on a 128-byte boundary
        oc.claimed = bs.claimed; bs.claimed += up64((px * 4 + 31) / 32);
        oc.mins = bs.mins; if (keepall) bs.mins += px * 4;
        l.n_oct = o + 1;
    }
    // capacities.  Candidates are DoG extrema with |DoG| > 20: a plateau of equal values is the worst case (every pixel a tied
    // extremum); 3 layers x sum_o px0 / 4^o <= 4 px0 is provisioned.  Refined points / keypoints must survive the contrast test.
    l.cand_cap = (unsigned)((4 * px0 + 1024 + NREG - 1) / NREG + ((size_t)MAX_OCT * 3 * EW * EH << REG_SHIFT) + 1024);   // + one full run of tiles per octave
    l.ref_cap = l.kp_cap = (unsigned)(px0 / 8 + 65536);
    l.cube_cap = std::min((unsigned)(px0 / 4 / NREG + 4096), l.cand_cap);
    bs.cand = (size_t)l.cand_cap * NREG; bs.refined = l.ref_cap; bs.kps = l.kp_cap; bs.cube = (size_t)l.cube_cap * NREG * 32;
    bs.sel = keepall ? (size_t)kmax : SEL_STRIDE;
    l.ksort_stride = keepall ? (size_t)((kmax + KA_TILE - 1) / KA_TILE) * KA_TILE : 0;
    return l;
}

int batch_frames(int w, int h, bool keepall, int requested, int slots, size_t total_mem) {
    int nb = std::min(std::max(requested, 1), BATCH_MAX);
    // A frame's work area is ~60 bytes per pixel (pyramid 16, worst-case candidate list 32, neighbourhood records 8, the rest 4);
    // keep-all: + 21 B per pixel of start keys
    const double per_frame = (keepall ? 1.4 : 1.0) * 60.0 * (double)w * (double)h;
    if (total_mem) nb = std::min(nb, std::max((int)(0.6 * (double)total_mem / per_frame / (double)slots), 1));
    return keepall ? std::min(nb, 8) : nb;
}

// Does this level go through blur16_stream?  Rows of whole 8-byte groups, last strip wider than the largest radius, enough columns (512;
// narrow: STREAM_NARROW_MIN_W, see sift_plan.h) and rows to fill the chip, a radius the kernel is instantiated for; the decimated copy needs R = 8 and an even height (the even rows of
// every segment are then the even rows of the image).
static bool blur_streams(const Routes& r, const Octave& oc, bool base, int R, bool ds) {
    const bool has_r = base ? R == 6 : (R == 5 || R == 6 || R == 8 || R == 10 || R == 13);
    return r.blur_stream && has_r && (oc.w & 3) == 0 && ((oc.w & 255) == 0 || (oc.w & 255) > MAX_R) && oc.w >= (r.narrow ? STREAM_NARROW_MIN_W : 512) && oc.h >= 64 &&
           (!base || r.base_frames_aligned) && (!ds || (R == 8 && (oc.h & 1) == 0));
}

// a launch of n frames of octave o; bpp: algorithmic bytes per pixel.  streamed(): a wave per unit, four to a block; tiled(): a grid row per frame
struct Maker {
    const Octave& oc; int n;
    Launch L;
    Maker(const Octave& oc_, int n_, int o, int level, double bpp) : oc(oc_), n(n_), L{} { L.octave = o; L.level = level; L.bytes = (double)oc.w * oc.h * n * bpp; }
    Launch streamed(Kind k) { L.kind = k; L.nseg = (oc.h + L.L - 1) / L.L; L.gx = (unsigned)(L.nstrip * L.nseg * n + 3) / 4; L.gy = L.gz = 1; return L; }
    Launch tiled(Kind k, int tw, int th) { L.kind = k; L.gx = (unsigned)(((oc.w + tw - 1) / tw) * ((oc.h + th - 1) / th)); L.gy = (unsigned)n; L.gz = 1; return L; }
};

static Launch blur_launch(const Routes& r, const Octave& oc, int n, int o, int level, bool ds) {
    const bool base = level == 0;
    Maker m(oc, n, o, level, base ? 5.0 : 4.0);      // base: read the u8 frames, write level 0; else one read + one write of the level
    Launch& L = m.L;
    L.ds = ds;
    L.radius = base ? pyramid_taps().base.r : pyramid_taps().lv[level].r;
    if (!blur_streams(r, oc, base, L.radius, ds)) return m.tiled(BLUR_TILE, T16W, T16H);
    // barrier-free streaming kernel over the whole chip in one round of `waves` per SIMD, segments of an even number of rows, all frames in one launch
    L.waves = L.radius <= STREAM_W4_MAX_R ? 4 : 3;
    L.nstrip = (oc.w + 255) / 256;
    const int units = L.nstrip * n, nseg = (WAVE_SLOTS * L.waves + units - 1) / units;
    const int rows = (oc.h + nseg - 1) / nseg;
    L.L = (std::max(rows, STREAM_MIN_L) + 1) & ~1;
    if (r.narrow && rows < STREAM_MIN_L) {
        // STREAM_MIN_L leaves SIMDs with one wave or none: shorter segments, STREAM_NARROW_WAVES waves on every SIMD
        const int nseg2 = (WAVE_SLOTS * STREAM_NARROW_WAVES + units - 1) / units;
        L.L = std::min((std::max((oc.h + nseg2 - 1) / nseg2, STREAM_NARROW_MIN_L) + 1) & ~1, L.L);
    }
    return m.streamed(BLUR_STREAM);
}

static Launch extrema_launch(const Routes& r, const Octave& oc, int n, int o) {
    Maker m(oc, n, o, -1, 12.0);      // the six levels read once
    Launch& L = m.L;
    // the streamed test pays off on the big octaves of a full batch; smaller launches do not keep enough rows in flight and stay with the tiled kernel
    if (!(r.blur_stream && (oc.w & 3) == 0 && oc.w >= r.xstream_min_w && oc.h >= r.xstream_min_w * 3 / 4 && n >= r.xstream_min_frames)) return m.tiled(EXTREMA_TILE, EW, EH);
    // no row halo to amortise here (3 + XD rows to prime a segment): many short segments balance the wave slots
    L.nstrip = (oc.w + XSW - 1) / XSW;
    L.xsw = ((oc.w + L.nstrip - 1) / L.nstrip + 3) & ~3;      // equal strips (<= 248 columns) instead of a nearly empty last one
    // whole rounds of the WAVE_SLOTS x XWAVES wave slots: the largest k <= 2 whose segments stay >= 64 rows
    L.L = oc.h;
    for (int k = 2; k >= 1; k--) {
        const int ns = (WAVE_SLOTS * XWAVES * k) / (L.nstrip * n);
        if (ns < 1) continue;
        const int l = (oc.h + ns - 1) / ns;
        if (l >= 64 || k == 1) { L.L = std::max(l, 64); break; }
    }
    return m.streamed(EXTREMA_STREAM);
}

std::vector<Launch> pyramid_launches(const Layout& l, int n, const Routes& r) {
    std::vector<Launch> out;
    bool ds_fused = false;
    for (int o = 0; o < l.n_oct; o++) {
        const Octave& oc = l.oc[o];
        if (o == 0) out.push_back(blur_launch(r, oc, n, 0, 0, false));      // base level straight from the caller's frames
        else if (!ds_fused) {
            Launch L = Maker(oc, n, o, 0, 4.0).L;
            L.kind = DOWNSAMPLE; L.gx = (unsigned)(oc.w + 63) / 64; L.gy = (unsigned)(oc.h + 3) / 4; L.gz = (unsigned)n;
            out.push_back(L);
        }
        for (int i = 1; i < N_LEVELS; i++) {
            // the level that seeds the next octave writes its decimation on the way out (saves re-reading it), unless only the copy
            // keeps the level from streaming (odd height): rather stream without it
            const int R = pyramid_taps().lv[i].r;
            bool ds = i == N_LAYERS && o + 1 < l.n_oct && (oc.w & 3) == 0;
            if (ds && !blur_streams(r, oc, false, R, true) && blur_streams(r, oc, false, R, false)) ds = false;
            if (i == N_LAYERS) ds_fused = ds;
            out.push_back(blur_launch(r, oc, n, o, i, ds));
        }
        out.push_back(extrema_launch(r, oc, n, o));
    }
    return out;
}

}  // namespace sift_plan
