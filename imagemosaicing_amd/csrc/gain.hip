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
    const double alpha = 1.0 / ((double)prm.sigma_n * (double)prm.sigma_n), beta = 1.0 / ((double)prm.sigma_g * (double)prm.sigma_g);
    // the frames with an equation and the graph of the pairs with n > 0 (the same for every channel)
    std::vector<char> active((size_t)n, 0);
    for (int k = 0; k < n; k++) if (cover[k] > 0) active[k] = 1;
    std::vector<int> live;                                    // pairs that add terms
    for (int p = 0; p < n_pairs; p++) if (ps[p].n > 0) { live.push_back(p); active[ps[p].a] = 1; active[ps[p].b] = 1; }
    std::vector<int> idx((size_t)n, -1), node;
    for (int k = 0; k < n; k++) if (active[k]) { idx[k] = (int)node.size(); node.push_back(k); }
    const int m = (int)node.size();
    for (int k = 0; k < n; k++) gains[3 * k] = gains[3 * k + 1] = gains[3 * k + 2] = 1.0f;
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
    std::vector<double> E(rp[m]), diag((size_t)m), rhs((size_t)m), x((size_t)m), r((size_t)m), d((size_t)m);
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
            if (!(s > 0.0)) { err = "the normal equations are not positive definite at frame " + std::to_string(node[order[i]]); return MI355_ERR_FAILED; }
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
            const float g = (float)x[pos[i]];
            if (nch == 3) gains[3 * node[i] + c] = g;
            else gains[3 * node[i]] = gains[3 * node[i] + 1] = gains[3 * node[i] + 2] = g;
        }
    }
    return MI355_OK;
}

int apply_gains(mi355_ctx* ctx, const uint8_t* const* d_src, uint8_t* const* d_dst, const int* w, const int* h, const int* ws, int n, const float* gains) {
    std::string err;
    if (!d_src || !d_dst || !w || !h || !ws || !gains) { ctx->set_error("apply_gains: NULL argument"); return MI355_ERR_ARG; }
    if (!check_frames_n(n, err)) { ctx->set_error("apply_gains: " + err); return MI355_ERR_ARG; }
    struct Span { uintptr_t lo, hi; int k; };
    std::vector<Span> dsts, srcs;
    for (int k = 0; k < n; k++) {
        const std::string fk = "apply_gains: frame " + std::to_string(k);
        if (!d_src[k] || !d_dst[k]) { ctx->set_error(fk + ": NULL pointer"); return MI355_ERR_ARG; }
        if (w[k] < 1 || h[k] < 1 || ws[k] < 3 * w[k]) { ctx->set_error(fk + ": bad geometry w=" + std::to_string(w[k]) + " h=" + std::to_string(h[k]) + " ws=" + std::to_string(ws[k])); return MI355_ERR_ARG; }
        for (int c = 0; c < 3; c++)
            if (!std::isfinite(gains[3 * k + c])) { ctx->set_error(fk + ": gain[" + std::to_string(c) + "] is not finite"); return MI355_ERR_ARG; }
        const size_t bytes = (size_t)ws[k] * (size_t)(h[k] - 1) + 3 * (size_t)w[k];
        dsts.push_back({(uintptr_t)d_dst[k], (uintptr_t)d_dst[k] + bytes, k});
        srcs.push_back({(uintptr_t)d_src[k], (uintptr_t)d_src[k] + bytes, k});
    }
    // a dst range may meet no other range but its own src range exactly
    std::sort(dsts.begin(), dsts.end(), [](const Span& x, const Span& y) { return x.lo < y.lo; });
    for (size_t i = 1; i < dsts.size(); i++)
        if (dsts[i].lo < dsts[i - 1].hi) { ctx->set_error("apply_gains: dst of frame " + std::to_string(dsts[i].k) + " overlaps dst of frame " + std::to_string(dsts[i - 1].k)); return MI355_ERR_ARG; }
    for (const Span& s : srcs) {
        auto it = std::lower_bound(dsts.begin(), dsts.end(), s.hi, [](const Span& x, uintptr_t v) { return x.lo < v; });   // first dst starting at or after s.hi
        if (it == dsts.begin()) continue;
        --it;                                                                                                              // the last dst starting before s.hi
        if (it->hi <= s.lo) continue;
        if (it->k == s.k && it->lo == s.lo) continue;                                                                      // in place
        ctx->set_error("apply_gains: dst of frame " + std::to_string(it->k) + " overlaps src of frame " + std::to_string(s.k) + " without being equal to it");
        return MI355_ERR_ARG;
    }
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
