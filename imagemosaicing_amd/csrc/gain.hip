// csrc/gain.hip -- exposure gain compensation (gfx950): per-frame, per-channel gains from the frames' overlaps, applied to the texels before a
// render (include/mi355_mosaic.h, "exposure gain compensation").  OpenCV's detail::GainCompensator restricted to the listed pairs, with the
// overlap means measured on a lattice of canvas pixels through the refined render's own map and sample (mosaic_frame.h).
//
//   gain_stats_kernel   the hot path.  The work list is built on the host: tiles of 64 x 16 lattice points, over each listed pair's
//                       canvas-box intersection (pair tiles) and over each frame's own box (cover tiles, for N_k).  One launch for all of
//                       them; one lane per lattice point column, 4 lattice rows per lane.  A pair tile maps the point into both frames and,
//                       where both have a sample, gathers both 2 x 2 neighbourhoods (load_quad3, the render's loads) and sums the bytes; a
//                       cover tile only maps and counts (no texel loads).  The sums are reduced in 32-bit registers (at most 256 x 4 x 255
//                       per field and workgroup) and land with one 64-bit vector atomic per field per workgroup in a device record array:
//                       integer sums, so the result does not depend on the order the workgroups run in.
//   gain_apply_kernel   a row-streaming LUT pass over every frame in one launch: a workgroup builds its frame's 3 x 256 table in LDS from
//                       the gains (in double) and streams 16 rows, 16 B in and 16 B out per lane where the row is aligned, bytes at the ends.
//                       Its roofline is HBM: 2 x 3 w h bytes per frame.
//   mi355_solve_gains   host, single-threaded double: the normal equations over the frames that have one, reverse Cuthill-McKee order, an
//                       envelope Cholesky factor and one step of iterative refinement.  Fixed order throughout: the same bits every call.
// Block gains (a gain map per frame on a grid of cells; header section "block gain compensation") follow further down with their own kernels;
// they share the work list, the map and sample, the node solve (solve_nodes) and the apply's frame check with the per-frame stage.
#include "common.h"
#include "hmath.h"
#include "mosaic_frame.h"
#include <algorithm>
#include <cmath>
#include <unordered_map>

namespace {

constexpr int GT_X = 64, GT_Y = 16;           // lattice columns x rows of a stats tile (256 lanes: 64 x 4, 4 rows each)
constexpr int AP_NT = 256, AP_ROWS = 16;      // apply: lanes and frame rows per workgroup
constexpr int GAIN_MAX_FRAMES = 65535;

struct GainTile { int a, b, rec; int lx0, ly0, lx1, ly1; int _pad; };   // b < 0: cover tile of frame a (rec = a); else pair record rec

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__global__ __launch_bounds__(256) void gain_stats_kernel(const FrameDev* fr, const GainTile* tiles, int step, float dGx, float dGy,
                                                         unsigned long long* pair_acc, unsigned long long* cover_acc) {
    const GainTile t = tiles[blockIdx.x];
    const int lx = t.lx0 + (threadIdx.x & 63), ly0 = t.ly0 + (threadIdx.x >> 6);
    const FrameDev& fa = fr[t.a];
    const float wa1 = (float)(fa.w - 1), ha1 = (float)(fa.h - 1);
    const float xf = (float)(lx * step) - dGx;                   // the render's xf = (float)xD - dGx
    const bool col = lx <= t.lx1;
    int v[7] = {0, 0, 0, 0, 0, 0, 0};                            // count, sum_a[3], sum_b[3]
    if (t.b < 0) {
#pragma unroll
        for (int r = 0; r < GT_Y / 4; r++) {
            const int ly = ly0 + 4 * r;
            const float yf = (float)(ly * step) - dGy;
            float xs, ys;
            frame_src(fa, xf, yf, xs, ys);
            v[0] += (col && ly <= t.ly1 && src_inside(xs, ys, wa1, ha1)) ? 1 : 0;
        }
    } else {
        const FrameDev& fb = fr[t.b];
        const float wb1 = (float)(fb.w - 1), hb1 = (float)(fb.h - 1);
#pragma unroll
        for (int r = 0; r < GT_Y / 4; r++) {
            const int ly = ly0 + 4 * r;
            const float yf = (float)(ly * step) - dGy;
            float xa, ya, xb, yb;
            frame_src(fa, xf, yf, xa, ya);
            frame_src(fb, xf, yf, xb, yb);
            if (col && ly <= t.ly1 && src_inside(xa, ya, wa1, ha1) && src_inside(xb, yb, wb1, hb1)) {
                unsigned b0, g0, r0, b1, g1, r1;
                frame_sample3(fa, xa, ya, b0, g0, r0);
                frame_sample3(fb, xb, yb, b1, g1, r1);
                v[0] += 1; v[1] += (int)b0; v[2] += (int)g0; v[3] += (int)r0; v[4] += (int)b1; v[5] += (int)g1; v[6] += (int)r1;
            }
        }
    }
    __shared__ int s_v[4][7];
    const int nv = t.b < 0 ? 1 : 7;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int i = 0; i < nv; i++) {
        const int s = wave_sum(v[i]);
        if (lane == 0) s_v[wave][i] = s;
    }
    __syncthreads();
    if (threadIdx.x < nv) {
        const int i = threadIdx.x;
        const long long s = (long long)s_v[0][i] + s_v[1][i] + s_v[2][i] + s_v[3][i];
        if (s != 0) {
            unsigned long long* dst = t.b < 0 ? cover_acc + t.rec : pair_acc + 7 * (size_t)t.rec + i;
            atomicAdd(dst, (unsigned long long)s);
        }
    }
}

struct ApplyFrame { const uint8_t* src; uint8_t* dst; int w, h, ws, first_block; float g[3]; int _pad; };

__global__ __launch_bounds__(AP_NT) void gain_apply_kernel(const ApplyFrame* frames, int nf) {
    __shared__ uint8_t lut[3 * 256];
    __shared__ int s_k;
    // the frame of this workgroup: the last k with first_block <= blockIdx.x (first_block ascends)
    if (threadIdx.x == 0) {
        int lo = 0, hi = nf - 1;
        while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (frames[mid].first_block <= (int)blockIdx.x) lo = mid; else hi = mid - 1; }
        s_k = lo;
    }
    __syncthreads();
    const ApplyFrame& f = frames[s_k];
    {
        const int v = threadIdx.x;                                  // AP_NT == 256: one table entry per lane and channel
#pragma unroll
        for (int c = 0; c < 3; c++) {
            double o = floor((double)f.g[c] * (double)v + 0.5);
            o = o < 0.0 ? 0.0 : (o > 255.0 ? 255.0 : o);
            lut[c * 256 + v] = (uint8_t)(int)o;
        }
    }
    __syncthreads();
    const int y0 = ((int)blockIdx.x - f.first_block) * AP_ROWS;
    const int nb = 3 * f.w;
    for (int y = y0; y < y0 + AP_ROWS && y < f.h; y++) {
        const uint8_t* srow = f.src + (size_t)y * f.ws;
        uint8_t* drow = f.dst + (size_t)y * f.ws;
        int head = (int)((16 - ((uintptr_t)srow & 15)) & 15);
        if (head > nb) head = nb;
        const bool vec = (((uintptr_t)(drow + head)) & 15) == 0;
        const int nvec = vec ? (nb - head) >> 4 : 0;
        const int tail = head + 16 * nvec;
        for (int i = threadIdx.x; i < nvec; i += AP_NT) {
            const int off = head + 16 * i;
            const uint4 in = *reinterpret_cast<const uint4*>(srow + off);
            const unsigned w4[4] = {in.x, in.y, in.z, in.w};
            unsigned o4[4];
            int c = off % 3;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                unsigned o = 0;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    o |= (unsigned)lut[c * 256 + ((w4[q] >> (8 * j)) & 0xffu)] << (8 * j);
                    c = c == 2 ? 0 : c + 1;
                }
                o4[q] = o;
            }
            *reinterpret_cast<uint4*>(drow + off) = make_uint4(o4[0], o4[1], o4[2], o4[3]);
        }
        // the row's ends (or the whole row where src and dst are not aligned alike): bytes
        const int nhead = vec ? head : nb;
        for (int i = threadIdx.x; i < nhead; i += AP_NT) drow[i] = lut[(i % 3) * 256 + srow[i]];
        if (vec)
            for (int i = tail + (int)threadIdx.x; i < nb; i += AP_NT) drow[i] = lut[(i % 3) * 256 + srow[i]];
    }
}

std::string pair_str(int p, int a, int b) { return "pair " + std::to_string(p) + " (" + std::to_string(a) + ", " + std::to_string(b) + ")"; }

// a == b, a position out of range, an unordered pair listed twice
bool check_pairs(const int32_t* ab, int n_pairs, int n, std::string& err) {
    std::unordered_map<uint64_t, int> seen;
    seen.reserve((size_t)n_pairs * 2 + 1);
    for (int p = 0; p < n_pairs; p++) {
        const int a = ab[2 * p], b = ab[2 * p + 1];
        if (a < 0 || a >= n || b < 0 || b >= n) { err = pair_str(p, a, b) + ": position outside [0, " + std::to_string(n) + ")"; return false; }
        if (a == b) { err = pair_str(p, a, b) + ": a == b"; return false; }
        const uint64_t key = ((uint64_t)std::min(a, b) << 32) | (uint64_t)std::max(a, b);
        auto it = seen.find(key);
        if (it != seen.end()) { err = pair_str(p, a, b) + " repeats pair " + std::to_string(it->second); return false; }
        seen.emplace(key, p);
    }
    return true;
}

bool check_frames_n(int n, std::string& err) {
    if (n < 1 || n > GAIN_MAX_FRAMES) { err = "n=" + std::to_string(n) + " outside [1, 65535]"; return false; }
    return true;
}

bool check_params(const mi355_gain_params& p, bool need_step, std::string& err) {
    if (need_step && (p.step < 1 || p.step > 64)) { err = "step=" + std::to_string(p.step) + " outside [1, 64]"; return false; }
    if (p.channels != 1 && p.channels != 3) { err = "channels=" + std::to_string(p.channels) + " (need 1 or 3)"; return false; }
    if (!(p.sigma_n > 0.0f) || !std::isfinite(p.sigma_n)) { err = "sigma_n=" + std::to_string(p.sigma_n) + " must be > 0"; return false; }
    if (!(p.sigma_g > 0.0f) || !std::isfinite(p.sigma_g)) { err = "sigma_g=" + std::to_string(p.sigma_g) + " must be > 0"; return false; }
    return true;
}

int lattice_lo(int x0, int step) { return (x0 + step - 1) / step; }       // x0 >= 0

void push_tiles(std::vector<GainTile>& tiles, int a, int b, int rec, int x0, int x1, int y0, int y1, int step) {
    const int lx0 = lattice_lo(x0, step), lx1 = x1 / step, ly0 = lattice_lo(y0, step), ly1 = y1 / step;
    if (lx0 > lx1 || ly0 > ly1) return;
    for (int ty = ly0; ty <= ly1; ty += GT_Y)
        for (int tx = lx0; tx <= lx1; tx += GT_X) {
            GainTile t;
            t.a = a; t.b = b; t.rec = rec; t.lx0 = tx; t.ly0 = ty;
            t.lx1 = std::min(tx + GT_X - 1, lx1); t.ly1 = std::min(ty + GT_Y - 1, ly1); t._pad = 0;
            tiles.push_back(t);
        }
}

int gain_stats(mi355_ctx* ctx, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
               const int32_t* pairs_ab, int n_pairs, int step, mi355_gain_pair_stats* pair_stats, int64_t* frame_cover) {
    std::string err;
    if (!d_imgs || !w || !h || !ws || !h9s || (n_pairs > 0 && (!pairs_ab || !pair_stats)) || n_pairs < 0) { ctx->set_error("gain_stats: NULL argument or n_pairs < 0"); return MI355_ERR_ARG; }
    if (!check_frames_n(n, err) || !check_pairs(pairs_ab, n_pairs, n, err)) { ctx->set_error("gain_stats: " + err); return MI355_ERR_ARG; }
    if (step < 1 || step > 64) { ctx->set_error("gain_stats: step=" + std::to_string(step) + " outside [1, 64]"); return MI355_ERR_ARG; }
    int cw, ch, cws; float dG[2];
    if (mi355_mosaic_layout(w, h, n, h9s, &cw, &ch, &cws, dG) != MI355_OK) { ctx->set_error("gain_stats: no image with h[8] != 0 / empty canvas"); return MI355_ERR_FAILED; }
    std::vector<FrameDev> fr((size_t)n);
    std::vector<char> part((size_t)n, 0);
    for (int k = 0; k < n; k++) {
        if (!mi_frame_dev_setup(h9s + 9 * k, w[k], h[k], dG, cw, ch, 0, ch, fr[k])) continue;
        if (w[k] < 2 || h[k] < 2 || ws[k] < 3 * w[k]) { ctx->set_error("gain_stats: frame " + std::to_string(k) + ": bad geometry w=" + std::to_string(w[k]) + " h=" + std::to_string(h[k]) + " ws=" + std::to_string(ws[k])); return MI355_ERR_ARG; }
        if (!d_imgs[k]) { ctx->set_error("gain_stats: frame " + std::to_string(k) + " takes part but its pointer is NULL"); return MI355_ERR_ARG; }
        fr[k].src = d_imgs[k]; fr[k].w = w[k]; fr[k].h = h[k]; fr[k].ws = ws[k];
        part[k] = 1;
    }
    std::vector<GainTile> tiles;
    for (int k = 0; k < n; k++)
        if (part[k]) push_tiles(tiles, k, -1, k, fr[k].begX, fr[k].endX, fr[k].begY, fr[k].endY, step);
    for (int p = 0; p < n_pairs; p++) {
        const int a = pairs_ab[2 * p], b = pairs_ab[2 * p + 1];
        if (!part[a] || !part[b]) continue;
        const FrameDev &A = fr[a], &B = fr[b];
        push_tiles(tiles, a, b, p, std::max(A.begX, B.begX), std::min(A.endX, B.endX), std::max(A.begY, B.begY), std::min(A.endY, B.endY), step);
    }
    const size_t n_acc = (size_t)n_pairs * 7 + (size_t)n;
    DevBuf& dfr = ctx->buf("gain_frames"); DevBuf& dt = ctx->buf("gain_tiles"); DevBuf& dacc = ctx->buf("gain_acc");
    MI_HIP(dfr.reserve(sizeof(FrameDev) * (size_t)n));
    MI_HIP(dt.reserve(sizeof(GainTile) * std::max<size_t>(tiles.size(), 1)));
    MI_HIP(dacc.reserve(sizeof(unsigned long long) * n_acc));
    MI_HIP(hipMemcpyAsync(dfr.p, fr.data(), sizeof(FrameDev) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    if (!tiles.empty()) MI_HIP(hipMemcpyAsync(dt.p, tiles.data(), sizeof(GainTile) * tiles.size(), hipMemcpyHostToDevice, ctx->stream));
    MI_HIP(hipMemsetAsync(dacc.p, 0, sizeof(unsigned long long) * n_acc, ctx->stream));
    unsigned long long* pair_acc = dacc.as<unsigned long long>();
    unsigned long long* cover_acc = pair_acc + (size_t)n_pairs * 7;
    for (size_t t0 = 0; t0 < tiles.size(); t0 += (size_t)1 << 30) {     // grid.x < 2^31
        const size_t nt = std::min(tiles.size() - t0, (size_t)1 << 30);
        ProfScope ps(ctx, "gain_stats", 0.0);
        hipLaunchKernelGGL(gain_stats_kernel, dim3((unsigned)nt), dim3(256), 0, ctx->stream, dfr.as<FrameDev>(), dt.as<GainTile>() + t0, step,
                           dG[0], dG[1], pair_acc, cover_acc);
        MI_HIP(hipGetLastError());
    }
    std::vector<unsigned long long> acc(n_acc);
    MI_HIP(hipMemcpyAsync(acc.data(), dacc.p, sizeof(unsigned long long) * n_acc, hipMemcpyDeviceToHost, ctx->stream));
    MI_HIP(hipStreamSynchronize(ctx->stream));                 // fr / tiles are locals
    for (int p = 0; p < n_pairs; p++) {
        mi355_gain_pair_stats& s = pair_stats[p];
        s.a = pairs_ab[2 * p]; s.b = pairs_ab[2 * p + 1];
        s.n = (int64_t)acc[7 * (size_t)p];
        for (int c = 0; c < 3; c++) { s.sum_a[c] = (int64_t)acc[7 * (size_t)p + 1 + c]; s.sum_b[c] = (int64_t)acc[7 * (size_t)p + 4 + c]; }
    }
    if (frame_cover)
        for (int k = 0; k < n; k++) frame_cover[k] = (int64_t)acc[(size_t)n_pairs * 7 + k];
    return MI355_OK;
}

// ---- host solve -----------------------------------------------------------------------------------------------------------------------
constexpr double ENVELOPE_WORK_MAX = 2e9;     // multiply-adds of one envelope factorisation above which solve_nodes may iterate instead
constexpr int PCG_MAX_ITER = 2000;

// One channel of solve_nodes by conjugate gradients with the diagonal as preconditioner, from x = 1, every sum in index or pair-list order.
// Unknowns are the active ones (positions in node); diag / off / rhs are the channel's system in pair-list order.
// The stop is a bound, not a guess.  Every pair term 2 alpha n (I_ab e_a - I_ba e_b)(...)^T is positive semidefinite, so A >= beta diag(M) with
// M_i = N_i + the n of i's live pairs (integers >= 1).  With e = x - x*, r = rhs - A x:  e^T A e = r^T A^-1 r <= sum r_i^2 / (beta M_i)  and
// e^T A e >= beta min(M) |e|_inf^2, hence |e|_inf <= sqrt(sum r_i^2 / (beta M_i) / (beta min M)).  The iteration ends when that bound, taken on
// the residual computed afresh from x, is below 5e-10 max|x| (so below 1e-9 |x*|_inf); a system on which double arithmetic cannot bring the
// residual that low (a weak prior on a large graph) is refused.
int solve_pcg(const mi355_gain_pair_stats* ps, const std::vector<int>& live, const std::vector<int>& idx, const std::vector<int>& node, const int64_t* cover,
              const std::vector<double>& diag, const std::vector<double>& off, const std::vector<double>& rhs, double beta, std::vector<double>& x,
              std::string& err) {
    const int m = (int)node.size();
    std::vector<double> M((size_t)m), r((size_t)m), z((size_t)m), p((size_t)m), Ap((size_t)m);
    for (int i = 0; i < m; i++) M[i] = (double)cover[node[i]];
    for (int q : live) { M[idx[ps[q].a]] += (double)ps[q].n; M[idx[ps[q].b]] += (double)ps[q].n; }
    double mmin = M[0];
    for (int i = 1; i < m; i++) mmin = std::min(mmin, M[i]);
    auto matvec = [&](const std::vector<double>& v, std::vector<double>& y) {
        for (int i = 0; i < m; i++) y[i] = diag[i] * v[i];
        for (size_t q = 0; q < live.size(); q++) {
            const int a = idx[ps[live[q]].a], b = idx[ps[live[q]].b];
            y[a] += off[q] * v[b]; y[b] += off[q] * v[a];
        }
    };
    auto dot = [&](const std::vector<double>& a, const std::vector<double>& b) { double s = 0.0; for (int i = 0; i < m; i++) s += a[i] * b[i]; return s; };
    auto error_bound = [&]() { double s = 0.0; for (int i = 0; i < m; i++) s += r[i] * r[i] / (beta * M[i]); return std::sqrt(s / (beta * mmin)); };
    auto restart = [&]() {                                     // r, z, p from x
        matvec(x, Ap);
        for (int i = 0; i < m; i++) { r[i] = rhs[i] - Ap[i]; z[i] = r[i] / diag[i]; p[i] = z[i]; }
        return dot(r, z);
    };
    std::fill(x.begin(), x.end(), 1.0);
    double rho = restart();
    for (int it = 0; it < PCG_MAX_ITER; it++) {
        double xmax = 0.0;
        for (int i = 0; i < m; i++) xmax = std::max(xmax, std::fabs(x[i]));
        if (error_bound() <= 2.5e-10 * xmax) {
            rho = restart();                                   // the recurrence's residual drifts from the true one: decide on the true one
            if (error_bound() <= 5e-10 * xmax) return MI355_OK;
        }
        matvec(p, Ap);
        const double a = rho / dot(p, Ap);
        for (int i = 0; i < m; i++) { x[i] += a * p[i]; r[i] -= a * Ap[i]; z[i] = r[i] / diag[i]; }
        const double rho2 = dot(r, z);
        const double b = rho2 / rho;
        for (int i = 0; i < m; i++) p[i] = z[i] + b * p[i];
        rho = rho2;
    }
    err = "the iterative solve of " + std::to_string(m) + " unknowns did not reach 1e-9 in " + std::to_string(PCG_MAX_ITER) + " steps (prior too weak for a graph this large)";
    return MI355_ERR_FAILED;
}

// The normal equations of the header over n unknowns ("frames" for mi355_solve_gains, the nodes (frame, cell) for the block gains): ps[p].a / .b
// are unknowns, cover[k] is N_k.  x3: n x 3 doubles, 1 for an unknown without an equation (channels == 1: the one value in all three).
// The factorisation is the envelope Cholesky below.  may_iterate (block gains only): where its envelope would cost more than ENVELOPE_WORK_MAX
// multiply-adds per channel, a Jacobi-preconditioned conjugate gradient in the same fixed order takes its place; it stops on a bound of the
// error that it can prove (see there) and fails rather than return less.  unit names an unknown in the messages.
int solve_nodes(const mi355_gain_pair_stats* ps, int n_pairs, const int64_t* cover, int n, const mi355_gain_params& prm, const char* unit, bool may_iterate,
                double* x3, std::string& err) {
    const double alpha = 1.0 / ((double)prm.sigma_n * (double)prm.sigma_n), beta = 1.0 / ((double)prm.sigma_g * (double)prm.sigma_g);
    // the frames with an equation and the graph of the pairs with n > 0 (the same for every channel)
    std::vector<char> active((size_t)n, 0);
    for (int k = 0; k < n; k++) if (cover[k] > 0) active[k] = 1;
    std::vector<int> live;                                    // pairs that add terms
    for (int p = 0; p < n_pairs; p++) if (ps[p].n > 0) { live.push_back(p); active[ps[p].a] = 1; active[ps[p].b] = 1; }
    std::vector<int> idx((size_t)n, -1), node;
    for (int k = 0; k < n; k++) if (active[k]) { idx[k] = (int)node.size(); node.push_back(k); }
    const int m = (int)node.size();
    std::fill(x3, x3 + 3 * (size_t)n, 1.0);
    if (m == 0) return MI355_OK;
    std::vector<std::vector<int>> adj((size_t)m);
    for (int p : live) { const int u = idx[ps[p].a], v = idx[ps[p].b]; adj[u].push_back(v); adj[v].push_back(u); }
    for (auto& l : adj) std::sort(l.begin(), l.end());
    // reverse Cuthill-McKee: per component, start at the unvisited node of least degree (lowest index on ties), neighbours by (degree, index)
    std::vector<int> order; order.reserve(m);
    std::vector<char> seen((size_t)m, 0);
    std::vector<int> by_deg(m);
    for (int i = 0; i < m; i++) by_deg[i] = i;
    std::stable_sort(by_deg.begin(), by_deg.end(), [&](int x, int y) { return adj[x].size() < adj[y].size(); });
    for (int s : by_deg) {
        if (seen[s]) continue;
        size_t head = order.size();
        order.push_back(s); seen[s] = 1;
        std::vector<int> nb;
        while (head < order.size()) {
            const int u = order[head++];
            nb.clear();
            for (int v : adj[u]) if (!seen[v]) { nb.push_back(v); seen[v] = 1; }
            std::stable_sort(nb.begin(), nb.end(), [&](int x, int y) { return adj[x].size() < adj[y].size(); });
            order.insert(order.end(), nb.begin(), nb.end());
        }
    }
    std::reverse(order.begin(), order.end());
    std::vector<int> pos((size_t)m);
    for (int i = 0; i < m; i++) pos[order[i]] = i;
    // envelope: row i (permuted) holds columns fst[i] .. i
    std::vector<int> fst((size_t)m);
    for (int i = 0; i < m; i++) { int f = i; for (int v : adj[order[i]]) f = std::min(f, pos[v]); fst[i] = f; }
    std::vector<size_t> rp((size_t)m + 1, 0);
    for (int i = 0; i < m; i++) rp[i + 1] = rp[i] + (size_t)(i - fst[i] + 1);
    double work = 0.0;
    for (int i = 0; i < m; i++) work += (double)(i - fst[i]) * (double)(i - fst[i]);
    const bool iterate = may_iterate && work > ENVELOPE_WORK_MAX;
    std::vector<double> E(iterate ? 0 : rp[m]), diag((size_t)m), rhs((size_t)m), x((size_t)m), r((size_t)m), d((size_t)m);
    std::vector<double> off((size_t)live.size());
    auto at = [&](int i, int j) -> double& { return E[rp[i] + (size_t)(j - fst[i])]; };   // j in [fst[i], i]
    const int nch = prm.channels;
    for (int c = 0; c < nch; c++) {
        // the normal equations in pair-list order
        for (int i = 0; i < m; i++) { diag[i] = beta * (double)cover[node[i]]; rhs[i] = beta * (double)cover[node[i]]; }
        for (size_t q = 0; q < live.size(); q++) {
            const mi355_gain_pair_stats& s = ps[live[q]];
            const double nn = (double)s.n;
            double Iab, Iba;
            if (nch == 3) { Iab = (double)s.sum_a[c] / nn; Iba = (double)s.sum_b[c] / nn; }
            else { Iab = (double)(s.sum_a[0] + s.sum_a[1] + s.sum_a[2]) / (3.0 * nn); Iba = (double)(s.sum_b[0] + s.sum_b[1] + s.sum_b[2]) / (3.0 * nn); }
            const int u = idx[s.a], v = idx[s.b];
            diag[u] += 2.0 * alpha * Iab * Iab * nn + beta * nn;
            diag[v] += 2.0 * alpha * Iba * Iba * nn + beta * nn;
            off[q] = -2.0 * alpha * Iab * Iba * nn;
            rhs[u] += beta * nn; rhs[v] += beta * nn;
        }
        if (iterate) {
            const int rc = solve_pcg(ps, live, idx, node, cover, diag, off, rhs, beta, x, err);
            if (rc != MI355_OK) return rc;
            for (int i = 0; i < m; i++) {
                if (nch == 3) x3[3 * (size_t)node[i] + c] = x[i];
                else x3[3 * (size_t)node[i]] = x3[3 * (size_t)node[i] + 1] = x3[3 * (size_t)node[i] + 2] = x[i];
            }
            continue;
        }
        std::fill(E.begin(), E.end(), 0.0);
        for (int i = 0; i < m; i++) at(pos[i], pos[i]) = diag[i];
        for (size_t q = 0; q < live.size(); q++) {
            const int u = pos[idx[ps[live[q]].a]], v = pos[idx[ps[live[q]].b]];
            if (u > v) at(u, v) += off[q]; else at(v, u) += off[q];
        }
        // envelope Cholesky, row by row
        for (int i = 0; i < m; i++) {
            for (int j = fst[i]; j < i; j++) {
                double s = at(i, j);
                for (int k = std::max(fst[i], fst[j]); k < j; k++) s -= at(i, k) * at(j, k);
                at(i, j) = s / at(j, j);
            }
            double s = at(i, i);
            for (int k = fst[i]; k < i; k++) s -= at(i, k) * at(i, k);
            if (!(s > 0.0)) { err = std::string("the normal equations are not positive definite at ") + unit + " " + std::to_string(node[order[i]]); return MI355_ERR_FAILED; }
            at(i, i) = std::sqrt(s);
        }
        auto lsolve = [&](std::vector<double>& b) {              // b := (L L^T)^-1 b, permuted positions
            for (int i = 0; i < m; i++) { double s = b[i]; for (int k = fst[i]; k < i; k++) s -= at(i, k) * b[k]; b[i] = s / at(i, i); }
            for (int i = m - 1; i >= 0; i--) { b[i] /= at(i, i); const double bi = b[i]; for (int k = fst[i]; k < i; k++) b[k] -= at(i, k) * bi; }
        };
        for (int i = 0; i < m; i++) x[pos[i]] = rhs[i];
        lsolve(x);
        // one step of iterative refinement on the unfactored system: r = rhs - A x
        for (int i = 0; i < m; i++) r[pos[i]] = rhs[i] - diag[i] * x[pos[i]];
        for (size_t q = 0; q < live.size(); q++) {
            const int u = pos[idx[ps[live[q]].a]], v = pos[idx[ps[live[q]].b]];
            r[u] -= off[q] * x[v]; r[v] -= off[q] * x[u];
        }
        d = r;
        lsolve(d);
        for (int i = 0; i < m; i++) x[i] += d[i];
        for (int i = 0; i < m; i++) {
            const double g = x[pos[i]];
            if (nch == 3) x3[3 * (size_t)node[i] + c] = g;
            else x3[3 * (size_t)node[i]] = x3[3 * (size_t)node[i] + 1] = x3[3 * (size_t)node[i] + 2] = g;
        }
    }
    return MI355_OK;
}

int solve_gains(const mi355_gain_pair_stats* ps, int n_pairs, const int64_t* cover, int n, const mi355_gain_params& prm, float* gains, std::string& err) {
    if (!check_frames_n(n, err) || !check_params(prm, false, err)) return MI355_ERR_ARG;
    if (n_pairs < 0 || (n_pairs > 0 && !ps) || !cover || !gains) { err = "NULL argument or n_pairs < 0"; return MI355_ERR_ARG; }
    {
        std::vector<int32_t> ab((size_t)n_pairs * 2);
        for (int p = 0; p < n_pairs; p++) { ab[2 * p] = ps[p].a; ab[2 * p + 1] = ps[p].b; }
        if (!check_pairs(ab.data(), n_pairs, n, err)) return MI355_ERR_ARG;
    }
    for (int p = 0; p < n_pairs; p++)
        if (ps[p].n < 0) { err = pair_str(p, ps[p].a, ps[p].b) + ": n=" + std::to_string(ps[p].n) + " < 0"; return MI355_ERR_ARG; }
    for (int k = 0; k < n; k++)
        if (cover[k] < 0) { err = "frame " + std::to_string(k) + ": frame_cover=" + std::to_string(cover[k]) + " < 0"; return MI355_ERR_ARG; }
    std::vector<double> x3((size_t)n * 3);
    const int rc = solve_nodes(ps, n_pairs, cover, n, prm, "frame", false, x3.data(), err);
    if (rc != MI355_OK) return rc;
    for (size_t i = 0; i < x3.size(); i++) gains[i] = (float)x3[i];
    return MI355_OK;
}

// What mi355_apply_gains_dev and mi355_apply_block_gains_dev ask of their frames (who prefixes the messages): pointers, geometry, finite gains
// (per_frame values each), and a dst range that meets no other range but its own src range exactly.
int check_apply_frames(mi355_ctx* ctx, const std::string& who, const uint8_t* const* d_src, uint8_t* const* d_dst, const int* w, const int* h, const int* ws,
                       int n, const float* gains, int per_frame) {
    struct Span { uintptr_t lo, hi; int k; };
    std::vector<Span> dsts, srcs;
    for (int k = 0; k < n; k++) {
        const std::string fk = who + ": frame " + std::to_string(k);
        if (!d_src[k] || !d_dst[k]) { ctx->set_error(fk + ": NULL pointer"); return MI355_ERR_ARG; }
        if (w[k] < 1 || h[k] < 1 || ws[k] < 3 * w[k]) { ctx->set_error(fk + ": bad geometry w=" + std::to_string(w[k]) + " h=" + std::to_string(h[k]) + " ws=" + std::to_string(ws[k])); return MI355_ERR_ARG; }
        for (int c = 0; c < per_frame; c++)
            if (!std::isfinite(gains[(size_t)per_frame * k + c])) { ctx->set_error(fk + ": gain[" + std::to_string(c) + "] is not finite"); return MI355_ERR_ARG; }
        const size_t bytes = (size_t)ws[k] * (size_t)(h[k] - 1) + 3 * (size_t)w[k];
        dsts.push_back({(uintptr_t)d_dst[k], (uintptr_t)d_dst[k] + bytes, k});
        srcs.push_back({(uintptr_t)d_src[k], (uintptr_t)d_src[k] + bytes, k});
    }
    // a dst range may meet no other range but its own src range exactly
    std::sort(dsts.begin(), dsts.end(), [](const Span& x, const Span& y) { return x.lo < y.lo; });
    for (size_t i = 1; i < dsts.size(); i++)
        if (dsts[i].lo < dsts[i - 1].hi) { ctx->set_error(who + ": dst of frame " + std::to_string(dsts[i].k) + " overlaps dst of frame " + std::to_string(dsts[i - 1].k)); return MI355_ERR_ARG; }
    for (const Span& s : srcs) {
        auto it = std::lower_bound(dsts.begin(), dsts.end(), s.hi, [](const Span& x, uintptr_t v) { return x.lo < v; });   // first dst starting at or after s.hi
        if (it == dsts.begin()) continue;
        --it;                                                                                                              // the last dst starting before s.hi
        if (it->hi <= s.lo) continue;
        if (it->k == s.k && it->lo == s.lo) continue;                                                                      // in place
        ctx->set_error(who + ": dst of frame " + std::to_string(it->k) + " overlaps src of frame " + std::to_string(s.k) + " without being equal to it");
        return MI355_ERR_ARG;
    }
    return MI355_OK;
}

int apply_gains(mi355_ctx* ctx, const uint8_t* const* d_src, uint8_t* const* d_dst, const int* w, const int* h, const int* ws, int n, const float* gains) {
    std::string err;
    if (!d_src || !d_dst || !w || !h || !ws || !gains) { ctx->set_error("apply_gains: NULL argument"); return MI355_ERR_ARG; }
    if (!check_frames_n(n, err)) { ctx->set_error("apply_gains: " + err); return MI355_ERR_ARG; }
    { const int rc = check_apply_frames(ctx, "apply_gains", d_src, d_dst, w, h, ws, n, gains, 3); if (rc != MI355_OK) return rc; }
    std::vector<ApplyFrame> af;
    int blocks = 0;
    double bytes = 0.0;
    for (int k = 0; k < n; k++) {
        const bool unit = gains[3 * k] == 1.0f && gains[3 * k + 1] == 1.0f && gains[3 * k + 2] == 1.0f;
        if (unit && d_src[k] == d_dst[k]) continue;                       // in place with gains 1: the bytes stay as they are
        ApplyFrame f;
        f.src = d_src[k]; f.dst = d_dst[k]; f.w = w[k]; f.h = h[k]; f.ws = ws[k]; f.first_block = blocks; f._pad = 0;
        for (int c = 0; c < 3; c++) f.g[c] = gains[3 * k + c];
        af.push_back(f);
        blocks += (h[k] + AP_ROWS - 1) / AP_ROWS;
        bytes += 6.0 * (double)w[k] * h[k];
    }
    if (af.empty()) return MI355_OK;
    DevBuf& daf = ctx->buf("gain_apply_frames");
    MI_HIP(daf.reserve(sizeof(ApplyFrame) * af.size()));
    MI_HIP(hipMemcpyAsync(daf.p, af.data(), sizeof(ApplyFrame) * af.size(), hipMemcpyHostToDevice, ctx->stream));
    {
        ProfScope ps(ctx, "gain_apply", bytes);
        hipLaunchKernelGGL(gain_apply_kernel, dim3(blocks), dim3(AP_NT), 0, ctx->stream, daf.as<ApplyFrame>(), (int)af.size());
        MI_HIP(hipGetLastError());
    }
    MI_HIP(hipStreamSynchronize(ctx->stream));                 // af is a local
    return MI355_OK;
}

// ---- block gains: a gain map per frame (include/mi355_mosaic.h, "block gain compensation") ------------------------------------------------
//   block_gain_stats_kernel    gain_stats_kernel's work list, map and samples; the sums are binned by (cell_a, cell_b).  A lane adds up its four
//                              points in registers while their key stays the same; a wave whose lanes all end with one and the same key (the
//                              usual tile: a cell is hundreds of canvas pixels wide) reduces with shuffles as gain_stats_kernel does, every
//                              other lane adds its run to an LDS table keyed by hashing (BG_SLOTS = 1024 slots for at most 1024 points of a
//                              tile, so a key always finds a slot), and the occupied slots land with one 64-bit vector atomic per field in the
//                              batch's dense table: 7 planes of pairs x cells^2 accumulators.  Pairs go in batches whose table fits
//                              BG_TABLE_BYTES.  Integer sums: the order of the workgroups does not matter.
//   block_gain_compact_kernel  the table's entries with n > 0 become records (order arbitrary: the host sorts them).  The record buffer holds
//                              sum over the batch's pairs of min(cells^2, lattice points of the pair's tiles), which no batch can exceed;
//                              the kernel checks the slot all the same and the launcher fails on the flag.
//   block_gain_apply_kernel    gain_apply_kernel's row streaming with the header's integer interpolation in the LUT's place: per workgroup the
//                              16 rows' R_i (grid_x x 3 each) and the columns' (i0, fx) in LDS, so the divisions happen once per 16 rows.
constexpr int BG_MAX_GRID = 16, BG_SLOTS = 1024, BG_MAX_SMOOTH = 8;
constexpr int BG_MAX_DIM = 1 << 20;
constexpr size_t BG_TABLE_BYTES = (size_t)32 << 20;
constexpr int BA_COLS = 8192;                   // widest frame whose column table fits; wider frames compute (i0, fx) per pixel

// (xi * g) / w for 0 <= xi < w <= 2^20 and g <= 16: the product is below 2^24, exact in float; the float quotient is off by at most one
__device__ __forceinline__ int bg_cell(int xi, int g, int w, float rw) {
    const int num = xi * g;
    int q = (int)((float)num * rw);
    const int r = num - q * w;
    q += r >= w ? 1 : (r < 0 ? -1 : 0);
    return q;
}

template <int NV>
__device__ __forceinline__ void bg_flush(int* s_key, int (*s_val)[BG_SLOTS], int key, const int (&v)[7]) {
    unsigned s = ((unsigned)key * 2654435761u) >> 22;                    // 10 bits
    for (;;) {
        const int old = atomicCAS(&s_key[s], -1, key);
        if (old == -1 || old == key) break;
        s = (s + 1) & (BG_SLOTS - 1);                                    // at most 1024 keys for 1024 slots: ends
    }
#pragma unroll
    for (int i = 0; i < NV; i++)
        if (v[i]) atomicAdd(&s_val[i][s], v[i]);
}

// the lanes' runs into the LDS table: whole waves with one key through shuffles, the rest lane by lane
template <int NV>
__device__ __forceinline__ void bg_finish(int* s_key, int (*s_val)[BG_SLOTS], int cur, bool flushed, int (&v)[7]) {
    if (!__any(flushed)) {
        const unsigned long long m = __ballot(cur >= 0);
        if (m) {
            const int k0 = __shfl(cur, __ffsll((long long)m) - 1);
            if (__all(cur < 0 || cur == k0)) {
#pragma unroll
                for (int i = 0; i < NV; i++) v[i] = wave_sum(v[i]);
                if ((threadIdx.x & 63) == 0) bg_flush<NV>(s_key, s_val, k0, v);
                cur = -1;
            }
        }
    }
    if (cur >= 0) bg_flush<NV>(s_key, s_val, cur, v);
}

__global__ __launch_bounds__(256) void block_gain_stats_kernel(const FrameDev* fr, const GainTile* tiles, int step, float dGx, float dGy, int gx, int gy,
                                                               unsigned long long* pair_acc, size_t plane, unsigned long long* cover_acc) {
    __shared__ int s_key[BG_SLOTS];
    __shared__ int s_val[7][BG_SLOTS];
    for (int i = threadIdx.x; i < BG_SLOTS; i += 256) {
        s_key[i] = -1;
#pragma unroll
        for (int f = 0; f < 7; f++) s_val[f][i] = 0;
    }
    __syncthreads();
    const GainTile t = tiles[blockIdx.x];
    const int lx = t.lx0 + (threadIdx.x & 63), ly0 = t.ly0 + (threadIdx.x >> 6);
    const FrameDev& fa = fr[t.a];
    const float wa1 = (float)(fa.w - 1), ha1 = (float)(fa.h - 1);
    const float rwa = 1.0f / (float)fa.w, rha = 1.0f / (float)fa.h;
    const float xf = (float)(lx * step) - dGx;                   // the render's xf = (float)xD - dGx
    const bool col = lx <= t.lx1;
    const int cells = gx * gy;
    int v[7] = {0, 0, 0, 0, 0, 0, 0};                            // count, sum_a[3], sum_b[3] of the lane's current key
    int cur = -1;
    bool flushed = false;
    if (t.b < 0) {
#pragma unroll
        for (int r = 0; r < GT_Y / 4; r++) {
            const int ly = ly0 + 4 * r;
            const float yf = (float)(ly * step) - dGy;
            float xs, ys;
            frame_src(fa, xf, yf, xs, ys);
            if (col && ly <= t.ly1 && src_inside(xs, ys, wa1, ha1)) {
                const int key = bg_cell((int)ys, gy, fa.h, rha) * gx + bg_cell((int)xs, gx, fa.w, rwa);
                if (cur >= 0 && key != cur) { bg_flush<1>(s_key, s_val, cur, v); v[0] = 0; flushed = true; }
                cur = key;
                v[0] += 1;
            }
        }
        bg_finish<1>(s_key, s_val, cur, flushed, v);
    } else {
        const FrameDev& fb = fr[t.b];
        const float wb1 = (float)(fb.w - 1), hb1 = (float)(fb.h - 1);
        const float rwb = 1.0f / (float)fb.w, rhb = 1.0f / (float)fb.h;
#pragma unroll
        for (int r = 0; r < GT_Y / 4; r++) {
            const int ly = ly0 + 4 * r;
            const float yf = (float)(ly * step) - dGy;
            float xa, ya, xb, yb;
            frame_src(fa, xf, yf, xa, ya);
            frame_src(fb, xf, yf, xb, yb);
            if (col && ly <= t.ly1 && src_inside(xa, ya, wa1, ha1) && src_inside(xb, yb, wb1, hb1)) {
                unsigned b0, g0, r0, b1, g1, r1;
                frame_sample3(fa, xa, ya, b0, g0, r0);
                frame_sample3(fb, xb, yb, b1, g1, r1);
                const int ca = bg_cell((int)ya, gy, fa.h, rha) * gx + bg_cell((int)xa, gx, fa.w, rwa);
                const int cb = bg_cell((int)yb, gy, fb.h, rhb) * gx + bg_cell((int)xb, gx, fb.w, rwb);
                const int key = ca * cells + cb;
                if (cur >= 0 && key != cur) {
                    bg_flush<7>(s_key, s_val, cur, v);
#pragma unroll
                    for (int i = 0; i < 7; i++) v[i] = 0;
                    flushed = true;
                }
                cur = key;
                v[0] += 1; v[1] += (int)b0; v[2] += (int)g0; v[3] += (int)r0; v[4] += (int)b1; v[5] += (int)g1; v[6] += (int)r1;
            }
        }
        bg_finish<7>(s_key, s_val, cur, flushed, v);
    }
    __syncthreads();
    const int nv = t.b < 0 ? 1 : 7;
    for (int s = threadIdx.x; s < BG_SLOTS; s += 256) {
        const int key = s_key[s];
        if (key < 0) continue;
        if (t.b < 0) { atomicAdd(cover_acc + (size_t)t.a * cells + key, (unsigned long long)s_val[0][s]); continue; }
        unsigned long long* dst = pair_acc + (size_t)t.rec * cells * cells + key;
        for (int i = 0; i < nv; i++) {
            const int x = s_val[i][s];
            if (x) atomicAdd(dst + (size_t)i * plane, (unsigned long long)x);
        }
    }
}

// counter[0]: records written (or wanted), counter[1]: a record found no room
__global__ __launch_bounds__(256) void block_gain_compact_kernel(const unsigned long long* acc, size_t plane, int cells, int pair0, mi355_block_gain_stats* out,
                                                                 unsigned cap, unsigned* counter) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool has = i < plane && acc[i] != 0;
    const unsigned long long m = __ballot(has);
    if (!m) return;
    const int lane = threadIdx.x & 63, lead = __ffsll((long long)m) - 1;
    unsigned base = 0;
    if (lane == lead) base = atomicAdd(counter, (unsigned)__popcll(m));
    base = __shfl(base, lead);
    if (!has) return;
    const unsigned slot = base + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
    if (slot >= cap) { counter[1] = 1u; return; }
    const size_t c2 = (size_t)cells * cells;
    const int key = (int)(i % c2);
    mi355_block_gain_stats r;
    r.pair = pair0 + (int)(i / c2); r.cell_a = key / cells; r.cell_b = key % cells; r.reserved = 0;
    r.n = (int64_t)acc[i];
    for (int c = 0; c < 3; c++) { r.sum_a[c] = (int64_t)acc[(size_t)(1 + c) * plane + i]; r.sum_b[c] = (int64_t)acc[(size_t)(4 + c) * plane + i]; }
    out[slot] = r;
}

struct BlockApplyFrame { const uint8_t* src; uint8_t* dst; int w, h, ws, first_block; int q_off; int _pad; };

// the header's i0 and fx (or j0 and fy) of pixel x along an axis of w pixels and g cells
__device__ __forceinline__ void bg_axis(int x, int g, int w, unsigned& i0, unsigned& f) {
    int num = (2 * x + 1) * g - w;
    const int top = 2 * w * (g - 1);
    num = num < 0 ? 0 : (num > top ? top : num);
    const unsigned d = 2u * (unsigned)w;
    i0 = (unsigned)num / d;
    f = (((unsigned)num - i0 * d) * 256u) / d;
}

__global__ __launch_bounds__(AP_NT) void block_gain_apply_kernel(const BlockApplyFrame* frames, int nf, const uint16_t* qs, int gx, int gy) {
    __shared__ uint16_t s_col[BA_COLS];                         // i0 << 8 | fx
    __shared__ uint32_t s_R[AP_ROWS][BG_MAX_GRID * 3];          // R_i of the workgroup's rows, [i][channel]
    __shared__ int s_k;
    if (threadIdx.x == 0) {
        int lo = 0, hi = nf - 1;
        while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (frames[mid].first_block <= (int)blockIdx.x) lo = mid; else hi = mid - 1; }
        s_k = lo;
    }
    __syncthreads();
    const BlockApplyFrame& f = frames[s_k];
    const int y0 = ((int)blockIdx.x - f.first_block) * AP_ROWS;
    const int g3 = gx * 3;
    for (int e = threadIdx.x; e < AP_ROWS * g3; e += AP_NT) {
        const int r = e / g3, ic = e - r * g3;
        if (y0 + r >= f.h) break;
        unsigned j0, fy;
        bg_axis(y0 + r, gy, f.h, j0, fy);
        const unsigned j1 = min(j0 + 1u, (unsigned)gy - 1u);
        const uint16_t* q = qs + f.q_off;
        s_R[r][ic] = (256u - fy) * q[j0 * g3 + ic] + fy * q[j1 * g3 + ic];
    }
    const bool table = f.w <= BA_COLS;
    if (table)
        for (int x = threadIdx.x; x < f.w; x += AP_NT) {
            unsigned i0, fx;
            bg_axis(x, gx, f.w, i0, fx);
            s_col[x] = (uint16_t)(i0 << 8 | fx);
        }
    __syncthreads();
    const int nb = 3 * f.w;
    const unsigned glast = (unsigned)gx - 1u;
    auto column = [&](int x, unsigned& o0, unsigned& o1, unsigned& fx) {      // offsets of R_i0, R_i1 in a row of s_R
        x = x < f.w ? x : f.w - 1;
        unsigned i0;
        if (table) { const unsigned e = s_col[x]; i0 = e >> 8; fx = e & 255u; }
        else bg_axis(x, gx, f.w, i0, fx);
        o0 = 3u * i0; o1 = 3u * min(i0 + 1u, glast);
    };
    auto gain = [&](const uint32_t* R, unsigned o0, unsigned o1, unsigned fx, int c, unsigned v) {
        const unsigned G = (256u - fx) * R[o0 + c] + fx * R[o1 + c];
        const unsigned o = (((G + 128u) >> 8) * v + (1u << 19)) >> 20;
        return o > 255u ? 255u : o;
    };
    auto byte_at = [&](const uint32_t* R, int i, unsigned v) {
        const int x = i / 3;
        unsigned o0, o1, fx;
        column(x, o0, o1, fx);
        return (uint8_t)gain(R, o0, o1, fx, i - 3 * x, v);
    };
    for (int y = y0; y < y0 + AP_ROWS && y < f.h; y++) {
        const uint32_t* R = s_R[y - y0];
        const uint8_t* srow = f.src + (size_t)y * f.ws;
        uint8_t* drow = f.dst + (size_t)y * f.ws;
        int head = (int)((16 - ((uintptr_t)srow & 15)) & 15);
        if (head > nb) head = nb;
        const bool vec = (((uintptr_t)(drow + head)) & 15) == 0;
        const int nvec = vec ? (nb - head) >> 4 : 0;
        const int tail = head + 16 * nvec;
        for (int i = threadIdx.x; i < nvec; i += AP_NT) {
            const int off = head + 16 * i;
            const uint4 in = *reinterpret_cast<const uint4*>(srow + off);
            const unsigned w4[4] = {in.x, in.y, in.z, in.w};
            unsigned o4[4];
            int x = off / 3, c = off - 3 * x;
            unsigned o0, o1, fx;
            column(x, o0, o1, fx);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                unsigned o = 0;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    o |= gain(R, o0, o1, fx, c, (w4[q] >> (8 * j)) & 0xffu) << (8 * j);
                    if (c == 2) { c = 0; x++; column(x, o0, o1, fx); } else c++;
                }
                o4[q] = o;
            }
            *reinterpret_cast<uint4*>(drow + off) = make_uint4(o4[0], o4[1], o4[2], o4[3]);
        }
        // the row's ends (or the whole row where src and dst are not aligned alike): bytes
        const int nhead = vec ? head : nb;
        for (int i = threadIdx.x; i < nhead; i += AP_NT) drow[i] = byte_at(R, i, srow[i]);
        if (vec)
            for (int i = tail + (int)threadIdx.x; i < nb; i += AP_NT) drow[i] = byte_at(R, i, srow[i]);
    }
}

bool check_grid(int gx, int gy, std::string& err) {
    if (gx < 1 || gx > BG_MAX_GRID || gy < 1 || gy > BG_MAX_GRID) { err = "grid " + std::to_string(gx) + "x" + std::to_string(gy) + " outside [1, 16] x [1, 16]"; return false; }
    return true;
}

bool check_block_params(const mi355_block_gain_params& p, bool need_step, std::string& err) {
    mi355_gain_params g;
    g.sigma_n = p.sigma_n; g.sigma_g = p.sigma_g; g.channels = p.channels; g.step = p.step;
    if (!check_params(g, need_step, err) || !check_grid(p.grid_x, p.grid_y, err)) return false;
    if (p.smooth < 0 || p.smooth > BG_MAX_SMOOTH) { err = "smooth=" + std::to_string(p.smooth) + " outside [0, 8]"; return false; }
    return true;
}

int block_gain_stats(mi355_ctx* ctx, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s, const int32_t* pairs_ab,
                     int n_pairs, int step, int gx, int gy, std::vector<mi355_block_gain_stats>& recs, int64_t* cell_cover) {
    const std::string who = "block_gain_stats: ";
    std::string err;
    recs.clear();
    if (!d_imgs || !w || !h || !ws || !h9s || (n_pairs > 0 && !pairs_ab) || n_pairs < 0) { ctx->set_error(who + "NULL argument or n_pairs < 0"); return MI355_ERR_ARG; }
    if (!check_frames_n(n, err) || !check_pairs(pairs_ab, n_pairs, n, err) || !check_grid(gx, gy, err)) { ctx->set_error(who + err); return MI355_ERR_ARG; }
    if (step < 1 || step > 64) { ctx->set_error(who + "step=" + std::to_string(step) + " outside [1, 64]"); return MI355_ERR_ARG; }
    int cw, ch, cws; float dG[2];
    if (mi355_mosaic_layout(w, h, n, h9s, &cw, &ch, &cws, dG) != MI355_OK) { ctx->set_error(who + "no image with h[8] != 0 / empty canvas"); return MI355_ERR_FAILED; }
    std::vector<FrameDev> fr((size_t)n);
    std::vector<char> part((size_t)n, 0);
    for (int k = 0; k < n; k++) {
        if (!mi_frame_dev_setup(h9s + 9 * k, w[k], h[k], dG, cw, ch, 0, ch, fr[k])) continue;
        const std::string fk = who + "frame " + std::to_string(k);
        if (w[k] < 2 || h[k] < 2 || ws[k] < 3 * w[k] || w[k] > BG_MAX_DIM || h[k] > BG_MAX_DIM) { ctx->set_error(fk + ": bad geometry w=" + std::to_string(w[k]) + " h=" + std::to_string(h[k]) + " ws=" + std::to_string(ws[k])); return MI355_ERR_ARG; }
        if (w[k] < gx || h[k] < gy) { ctx->set_error(fk + " (" + std::to_string(w[k]) + "x" + std::to_string(h[k]) + ") is smaller than the " + std::to_string(gx) + "x" + std::to_string(gy) + " grid"); return MI355_ERR_ARG; }
        if (!d_imgs[k]) { ctx->set_error(fk + " takes part but its pointer is NULL"); return MI355_ERR_ARG; }
        fr[k].src = d_imgs[k]; fr[k].w = w[k]; fr[k].h = h[k]; fr[k].ws = ws[k];
        part[k] = 1;
    }
    const int cells = gx * gy;
    const size_t c2 = (size_t)cells * cells;
    const int per_batch = (int)std::max<size_t>(1, BG_TABLE_BYTES / (c2 * 7 * sizeof(unsigned long long)));
    const size_t n_cover = (size_t)n * cells;
    DevBuf& dfr = ctx->buf("gain_frames"); DevBuf& dt = ctx->buf("gain_tiles"); DevBuf& dacc = ctx->buf("block_gain_acc");
    DevBuf& dcov = ctx->buf("block_gain_cover"); DevBuf& dout = ctx->buf("block_gain_records"); DevBuf& dcnt = ctx->buf("block_gain_count");
    MI_HIP(dfr.reserve(sizeof(FrameDev) * (size_t)n));
    MI_HIP(dcov.reserve(sizeof(unsigned long long) * n_cover));
    MI_HIP(dcnt.reserve(2 * sizeof(unsigned)));
    MI_HIP(hipMemcpyAsync(dfr.p, fr.data(), sizeof(FrameDev) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    MI_HIP(hipMemsetAsync(dcov.p, 0, sizeof(unsigned long long) * n_cover, ctx->stream));
    std::vector<GainTile> tiles;
    for (int p0 = 0; p0 == 0 || p0 < n_pairs; p0 += per_batch) {
        const int np = std::min(per_batch, n_pairs - p0);
        const size_t plane = (size_t)std::max(np, 0) * c2;
        tiles.clear();
        if (p0 == 0)
            for (int k = 0; k < n; k++)
                if (part[k]) push_tiles(tiles, k, -1, k, fr[k].begX, fr[k].endX, fr[k].begY, fr[k].endY, step);
        size_t cap = 0;                                                // records this batch can give
        for (int p = p0; p < p0 + np; p++) {
            const int a = pairs_ab[2 * p], b = pairs_ab[2 * p + 1];
            if (!part[a] || !part[b]) continue;
            const FrameDev &A = fr[a], &B = fr[b];
            const size_t t0 = tiles.size();
            push_tiles(tiles, a, b, p - p0, std::max(A.begX, B.begX), std::min(A.endX, B.endX), std::max(A.begY, B.begY), std::min(A.endY, B.endY), step);
            size_t pts = 0;
            for (size_t t = t0; t < tiles.size(); t++) pts += (size_t)(tiles[t].lx1 - tiles[t].lx0 + 1) * (size_t)(tiles[t].ly1 - tiles[t].ly0 + 1);
            cap += std::min(pts, c2);
        }
        if (tiles.empty()) continue;
        if (tiles.size() >= ((size_t)1 << 31) || cap >= ((size_t)1 << 32)) { ctx->set_error(who + "too many tiles or records in one batch"); return MI355_ERR_FAILED; }
        MI_HIP(dt.reserve(sizeof(GainTile) * tiles.size()));
        MI_HIP(dacc.reserve(sizeof(unsigned long long) * std::max<size_t>(7 * plane, 1)));
        MI_HIP(dout.reserve(sizeof(mi355_block_gain_stats) * std::max<size_t>(cap, 1)));
        MI_HIP(hipMemcpyAsync(dt.p, tiles.data(), sizeof(GainTile) * tiles.size(), hipMemcpyHostToDevice, ctx->stream));
        if (plane) MI_HIP(hipMemsetAsync(dacc.p, 0, sizeof(unsigned long long) * 7 * plane, ctx->stream));
        MI_HIP(hipMemsetAsync(dcnt.p, 0, 2 * sizeof(unsigned), ctx->stream));
        {
            ProfScope ps(ctx, "block_gain_stats", 0.0);
            hipLaunchKernelGGL(block_gain_stats_kernel, dim3((unsigned)tiles.size()), dim3(256), 0, ctx->stream, dfr.as<FrameDev>(), dt.as<GainTile>(), step,
                               dG[0], dG[1], gx, gy, dacc.as<unsigned long long>(), plane, dcov.as<unsigned long long>());
            MI_HIP(hipGetLastError());
        }
        unsigned cnt[2] = {0, 0};
        if (plane && cap) {
            ProfScope ps(ctx, "block_gain_compact", (double)plane * 8.0);
            hipLaunchKernelGGL(block_gain_compact_kernel, dim3((unsigned)((plane + 255) / 256)), dim3(256), 0, ctx->stream, dacc.as<unsigned long long>(), plane,
                               cells, p0, dout.as<mi355_block_gain_stats>(), (unsigned)cap, dcnt.as<unsigned>());
            MI_HIP(hipGetLastError());
        }
        MI_HIP(hipMemcpyAsync(cnt, dcnt.p, sizeof(cnt), hipMemcpyDeviceToHost, ctx->stream));
        MI_HIP(hipStreamSynchronize(ctx->stream));                 // tiles is reused by the next batch
        if (cnt[1] || cnt[0] > cap) { ctx->set_error(who + "record buffer too small (" + std::to_string(cnt[0]) + " records for " + std::to_string(cap) + ")"); return MI355_ERR_FAILED; }
        if (cnt[0]) {
            const size_t at = recs.size();
            recs.resize(at + cnt[0]);
            MI_HIP(hipMemcpyAsync(recs.data() + at, dout.p, sizeof(mi355_block_gain_stats) * cnt[0], hipMemcpyDeviceToHost, ctx->stream));
            MI_HIP(hipStreamSynchronize(ctx->stream));
        }
    }
    std::sort(recs.begin(), recs.end(), [](const mi355_block_gain_stats& x, const mi355_block_gain_stats& y) {
        return x.pair != y.pair ? x.pair < y.pair : (x.cell_a != y.cell_a ? x.cell_a < y.cell_a : x.cell_b < y.cell_b);
    });
    if (cell_cover) {
        std::vector<unsigned long long> cov(n_cover);
        MI_HIP(hipMemcpyAsync(cov.data(), dcov.p, sizeof(unsigned long long) * n_cover, hipMemcpyDeviceToHost, ctx->stream));
        MI_HIP(hipStreamSynchronize(ctx->stream));
        for (size_t i = 0; i < n_cover; i++) cell_cover[i] = (int64_t)cov[i];
    } else MI_HIP(hipStreamSynchronize(ctx->stream));
    return MI355_OK;
}

int solve_block_gains(const mi355_block_gain_stats* rs, int64_t n_recs, const int32_t* pairs_ab, int n_pairs, const int64_t* cell_cover, int n,
                      const mi355_block_gain_params& prm, float* gains, std::string& err) {
    if (!check_frames_n(n, err) || !check_block_params(prm, false, err)) return MI355_ERR_ARG;
    if (n_recs < 0 || n_pairs < 0 || (n_recs > 0 && !rs) || (n_pairs > 0 && !pairs_ab) || !cell_cover || !gains) { err = "NULL argument or a count < 0"; return MI355_ERR_ARG; }
    if (!check_pairs(pairs_ab, n_pairs, n, err)) return MI355_ERR_ARG;
    const int gx = prm.grid_x, gy = prm.grid_y, cells = gx * gy;
    if (n_recs > (int64_t)0x7fffffff) { err = "n_records=" + std::to_string(n_recs) + " too large"; return MI355_ERR_ARG; }
    std::vector<mi355_gain_pair_stats> edges((size_t)n_recs);
    for (int64_t i = 0; i < n_recs; i++) {
        const mi355_block_gain_stats& r = rs[i];
        const std::string ri = "record " + std::to_string(i);
        if (r.pair < 0 || r.pair >= n_pairs) { err = ri + ": pair=" + std::to_string(r.pair) + " outside [0, " + std::to_string(n_pairs) + ")"; return MI355_ERR_ARG; }
        if (r.cell_a < 0 || r.cell_a >= cells || r.cell_b < 0 || r.cell_b >= cells) { err = ri + ": cell (" + std::to_string(r.cell_a) + ", " + std::to_string(r.cell_b) + ") outside [0, " + std::to_string(cells) + ")"; return MI355_ERR_ARG; }
        if (r.n < 0) { err = ri + ": n=" + std::to_string(r.n) + " < 0"; return MI355_ERR_ARG; }
        mi355_gain_pair_stats& e = edges[(size_t)i];
        e.a = pairs_ab[2 * r.pair] * cells + r.cell_a; e.b = pairs_ab[2 * r.pair + 1] * cells + r.cell_b; e.n = r.n;
        for (int c = 0; c < 3; c++) { e.sum_a[c] = r.sum_a[c]; e.sum_b[c] = r.sum_b[c]; }
    }
    const int nodes = n * cells;
    for (int i = 0; i < nodes; i++)
        if (cell_cover[i] < 0) { err = "frame " + std::to_string(i / cells) + " cell " + std::to_string(i % cells) + ": cell_cover=" + std::to_string(cell_cover[i]) + " < 0"; return MI355_ERR_ARG; }
    mi355_gain_params gp;
    gp.sigma_n = prm.sigma_n; gp.sigma_g = prm.sigma_g; gp.channels = prm.channels; gp.step = prm.step;
    std::vector<double> x3((size_t)nodes * 3);
    const int rc = solve_nodes(edges.data(), (int)n_recs, cell_cover, nodes, gp, "node", true, x3.data(), err);
    if (rc != MI355_OK) return rc;
    // smoothing: per frame and channel, x then y, edges replicated
    std::vector<double> a((size_t)cells), b((size_t)cells);
    for (int k = 0; k < n; k++)
        for (int c = 0; c < 3; c++) {
            double* m = x3.data() + (size_t)k * cells * 3 + c;           // m[3 * cell]
            for (int i = 0; i < cells; i++) a[i] = m[3 * i];
            for (int s = 0; s < prm.smooth; s++) {
                for (int y = 0; y < gy; y++)
                    for (int x = 0; x < gx; x++)
                        b[y * gx + x] = 0.25 * a[y * gx + std::max(x - 1, 0)] + 0.5 * a[y * gx + x] + 0.25 * a[y * gx + std::min(x + 1, gx - 1)];
                for (int y = 0; y < gy; y++)
                    for (int x = 0; x < gx; x++)
                        a[y * gx + x] = 0.25 * b[std::max(y - 1, 0) * gx + x] + 0.5 * b[y * gx + x] + 0.25 * b[std::min(y + 1, gy - 1) * gx + x];
            }
            for (int i = 0; i < cells; i++) gains[((size_t)k * cells + i) * 3 + c] = (float)a[i];
        }
    return MI355_OK;
}

int apply_block_gains(mi355_ctx* ctx, const uint8_t* const* d_src, uint8_t* const* d_dst, const int* w, const int* h, const int* ws, int n, int gx, int gy,
                      const float* gains) {
    const std::string who = "apply_block_gains";
    std::string err;
    if (!d_src || !d_dst || !w || !h || !ws || !gains) { ctx->set_error(who + ": NULL argument"); return MI355_ERR_ARG; }
    if (!check_frames_n(n, err) || !check_grid(gx, gy, err)) { ctx->set_error(who + ": " + err); return MI355_ERR_ARG; }
    const int per = gx * gy * 3;
    { const int rc = check_apply_frames(ctx, who, d_src, d_dst, w, h, ws, n, gains, per); if (rc != MI355_OK) return rc; }
    for (int k = 0; k < n; k++)
        if (w[k] > BG_MAX_DIM || h[k] > BG_MAX_DIM) { ctx->set_error(who + ": frame " + std::to_string(k) + ": w=" + std::to_string(w[k]) + " h=" + std::to_string(h[k]) + " above 2^20"); return MI355_ERR_ARG; }
    std::vector<BlockApplyFrame> af;
    std::vector<uint16_t> qs;
    int blocks = 0;
    double bytes = 0.0;
    for (int k = 0; k < n; k++) {
        const float* g = gains + (size_t)per * k;
        bool unit = true;
        for (int i = 0; i < per; i++) unit = unit && g[i] == 1.0f;
        if (unit && d_src[k] == d_dst[k]) continue;                       // in place with a map of 1: the bytes stay as they are
        BlockApplyFrame f;
        f.src = d_src[k]; f.dst = d_dst[k]; f.w = w[k]; f.h = h[k]; f.ws = ws[k]; f.first_block = blocks; f.q_off = (int)qs.size(); f._pad = 0;
        for (int i = 0; i < per; i++) {
            double q = std::floor((double)g[i] * 4096.0 + 0.5);
            q = q < 0.0 ? 0.0 : (q > 32767.0 ? 32767.0 : q);
            qs.push_back((uint16_t)(int)q);
        }
        af.push_back(f);
        blocks += (h[k] + AP_ROWS - 1) / AP_ROWS;
        bytes += 6.0 * (double)w[k] * h[k];
    }
    if (af.empty()) return MI355_OK;
    DevBuf& daf = ctx->buf("block_gain_apply_frames"); DevBuf& dq = ctx->buf("block_gain_apply_q");
    MI_HIP(daf.reserve(sizeof(BlockApplyFrame) * af.size()));
    MI_HIP(dq.reserve(sizeof(uint16_t) * qs.size()));
    MI_HIP(hipMemcpyAsync(daf.p, af.data(), sizeof(BlockApplyFrame) * af.size(), hipMemcpyHostToDevice, ctx->stream));
    MI_HIP(hipMemcpyAsync(dq.p, qs.data(), sizeof(uint16_t) * qs.size(), hipMemcpyHostToDevice, ctx->stream));
    {
        ProfScope ps(ctx, "block_gain_apply", bytes);
        hipLaunchKernelGGL(block_gain_apply_kernel, dim3(blocks), dim3(AP_NT), 0, ctx->stream, daf.as<BlockApplyFrame>(), (int)af.size(), dq.as<uint16_t>(), gx, gy);
        MI_HIP(hipGetLastError());
    }
    MI_HIP(hipStreamSynchronize(ctx->stream));                 // af, qs are locals
    return MI355_OK;
}

}  // namespace

extern "C" void mi355_default_gain_params(mi355_gain_params* p) {
    if (!p) return;
    p->sigma_n = 10.0f; p->sigma_g = 0.1f; p->channels = 3; p->step = 8;
}

extern "C" int mi355_gain_stats_dev(mi355_ctx* ctx, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                                    const int32_t* pairs_ab, int n_pairs, int step, mi355_gain_pair_stats* pair_stats, int64_t* frame_cover) {
    LOCKED_PROLOGUE
    return gain_stats(ctx, d_imgs, w, h, ws, n, h9s, pairs_ab, n_pairs, step, pair_stats, frame_cover);
}

extern "C" int mi355_solve_gains(const mi355_gain_pair_stats* pair_stats, int n_pairs, const int64_t* frame_cover, int n, const mi355_gain_params* p,
                                 float* gains) {
    mi355_gain_params dp;
    if (!p) { mi355_default_gain_params(&dp); p = &dp; }
    std::string err;
    const int rc = solve_gains(pair_stats, n_pairs, frame_cover, n, *p, gains, err);
    if (rc != MI355_OK) mi_set_host_error("solve_gains: " + err);
    return rc;
}

extern "C" int mi355_apply_gains_dev(mi355_ctx* ctx, const uint8_t* const* d_src, uint8_t* const* d_dst, const int* w, const int* h, const int* ws, int n,
                                     const float* gains) {
    LOCKED_PROLOGUE
    return apply_gains(ctx, d_src, d_dst, w, h, ws, n, gains);
}

extern "C" int mi355_gain_compensate_dev(mi355_ctx* ctx, uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                                         const int32_t* pairs_ab, int n_pairs, const mi355_gain_params* p, float* gains_out) {
    LOCKED_PROLOGUE
    mi355_gain_params dp;
    if (!p) { mi355_default_gain_params(&dp); p = &dp; }
    std::string err;
    if (!check_params(*p, true, err)) { ctx->set_error("gain_compensate: " + err); return MI355_ERR_ARG; }
    if (!check_frames_n(n, err)) { ctx->set_error("gain_compensate: " + err); return MI355_ERR_ARG; }
    std::vector<mi355_gain_pair_stats> st((size_t)std::max(n_pairs, 1));
    std::vector<int64_t> cover((size_t)n);
    int rc = gain_stats(ctx, (const uint8_t* const*)d_imgs, w, h, ws, n, h9s, pairs_ab, n_pairs, p->step, st.data(), cover.data());
    if (rc != MI355_OK) return rc;
    std::vector<float> g((size_t)n * 3);
    rc = solve_gains(st.data(), n_pairs, cover.data(), n, *p, g.data(), err);
    if (rc != MI355_OK) { ctx->set_error("gain_compensate: " + err); return rc; }
    // frames the render skips keep gain 1 and are not touched (their pointers may be NULL)
    std::vector<const uint8_t*> src((size_t)n);
    std::vector<uint8_t*> dst((size_t)n);
    std::vector<int> ww((size_t)n), hh((size_t)n), ss((size_t)n);
    std::vector<float> gg;
    int m = 0;
    for (int k = 0; k < n; k++) {
        if (g[3 * k] == 1.0f && g[3 * k + 1] == 1.0f && g[3 * k + 2] == 1.0f) continue;
        src[m] = d_imgs[k]; dst[m] = d_imgs[k]; ww[m] = w[k]; hh[m] = h[k]; ss[m] = ws[k];
        gg.insert(gg.end(), g.begin() + 3 * k, g.begin() + 3 * k + 3);
        m++;
    }
    if (m > 0) { rc = apply_gains(ctx, src.data(), dst.data(), ww.data(), hh.data(), ss.data(), m, gg.data()); if (rc != MI355_OK) return rc; }
    if (gains_out) std::copy(g.begin(), g.end(), gains_out);
    return MI355_OK;
}

extern "C" void mi355_default_block_gain_params(mi355_block_gain_params* p) {
    if (!p) return;
    p->sigma_n = 10.0f; p->sigma_g = 0.1f; p->channels = 3; p->step = 8; p->grid_x = 8; p->grid_y = 6; p->smooth = 2; p->reserved = 0;
}

extern "C" int mi355_block_gain_stats_dev(mi355_ctx* ctx, const uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                                          const int32_t* pairs_ab, int n_pairs, int step, int grid_x, int grid_y, mi355_block_gain_stats** records,
                                          int64_t* n_records, int64_t* cell_cover) {
    LOCKED_PROLOGUE
    if (!records || !n_records) { ctx->set_error("block_gain_stats: NULL argument or n_pairs < 0"); return MI355_ERR_ARG; }
    *records = nullptr; *n_records = 0;
    std::vector<mi355_block_gain_stats> recs;
    const int rc = block_gain_stats(ctx, d_imgs, w, h, ws, n, h9s, pairs_ab, n_pairs, step, grid_x, grid_y, recs, cell_cover);
    if (rc != MI355_OK || recs.empty()) return rc;
    mi355_block_gain_stats* out = (mi355_block_gain_stats*)malloc(sizeof(mi355_block_gain_stats) * recs.size());
    if (!out) { ctx->set_error("block_gain_stats: out of host memory"); return MI355_ERR_FAILED; }
    std::copy(recs.begin(), recs.end(), out);
    *records = out; *n_records = (int64_t)recs.size();
    return MI355_OK;
}

extern "C" int mi355_solve_block_gains(const mi355_block_gain_stats* records, int64_t n_records, const int32_t* pairs_ab, int n_pairs, const int64_t* cell_cover,
                                       int n, const mi355_block_gain_params* p, float* gains) {
    mi355_block_gain_params dp;
    if (!p) { mi355_default_block_gain_params(&dp); p = &dp; }
    std::string err;
    const int rc = solve_block_gains(records, n_records, pairs_ab, n_pairs, cell_cover, n, *p, gains, err);
    if (rc != MI355_OK) mi_set_host_error("solve_block_gains: " + err);
    return rc;
}

extern "C" int mi355_apply_block_gains_dev(mi355_ctx* ctx, const uint8_t* const* d_src, uint8_t* const* d_dst, const int* w, const int* h, const int* ws, int n,
                                           int grid_x, int grid_y, const float* gains) {
    LOCKED_PROLOGUE
    return apply_block_gains(ctx, d_src, d_dst, w, h, ws, n, grid_x, grid_y, gains);
}

extern "C" int mi355_block_gain_compensate_dev(mi355_ctx* ctx, uint8_t* const* d_imgs, const int* w, const int* h, const int* ws, int n, const float* h9s,
                                               const int32_t* pairs_ab, int n_pairs, const mi355_block_gain_params* p, float* gains_out) {
    LOCKED_PROLOGUE
    mi355_block_gain_params dp;
    if (!p) { mi355_default_block_gain_params(&dp); p = &dp; }
    std::string err;
    if (!check_block_params(*p, true, err) || !check_frames_n(n, err)) { ctx->set_error("block_gain_compensate: " + err); return MI355_ERR_ARG; }
    const int per = p->grid_x * p->grid_y * 3;
    std::vector<mi355_block_gain_stats> recs;
    std::vector<int64_t> cover((size_t)n * (per / 3));
    int rc = block_gain_stats(ctx, (const uint8_t* const*)d_imgs, w, h, ws, n, h9s, pairs_ab, n_pairs, p->step, p->grid_x, p->grid_y, recs, cover.data());
    if (rc != MI355_OK) return rc;
    std::vector<float> g((size_t)n * per);
    rc = solve_block_gains(recs.data(), (int64_t)recs.size(), pairs_ab, n_pairs, cover.data(), n, *p, g.data(), err);
    if (rc != MI355_OK) { ctx->set_error("block_gain_compensate: " + err); return rc; }
    // frames the render skips keep a map of 1 and are not touched (their pointers may be NULL)
    std::vector<const uint8_t*> src;
    std::vector<uint8_t*> dst;
    std::vector<int> ww, hh, ss;
    std::vector<float> gg;
    for (int k = 0; k < n; k++) {
        bool unit = true;
        for (int i = 0; i < per; i++) unit = unit && g[(size_t)per * k + i] == 1.0f;
        if (unit) continue;
        src.push_back(d_imgs[k]); dst.push_back(d_imgs[k]); ww.push_back(w[k]); hh.push_back(h[k]); ss.push_back(ws[k]);
        gg.insert(gg.end(), g.begin() + (size_t)per * k, g.begin() + (size_t)per * (k + 1));
    }
    if (!src.empty()) { rc = apply_block_gains(ctx, src.data(), dst.data(), ww.data(), hh.data(), ss.data(), (int)src.size(), p->grid_x, p->grid_y, gg.data()); if (rc != MI355_OK) return rc; }
    if (gains_out) std::copy(g.begin(), g.end(), gains_out);
    return MI355_OK;
}
