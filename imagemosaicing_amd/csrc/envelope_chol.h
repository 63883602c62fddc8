// csrc/envelope_chol.h -- the envelope (profile) Cholesky of the host alignments: the panel factorisation and the two triangular solves that
// mi355_global_affine_align* (host_io.cpp, 3 rows per image, two right-hand sides) and mi355_global_projective_refine* (projective_solve.cpp,
// 8 rows per image, one right-hand side) share.  Header-only: every host unit that includes it links on its own.  The matrix is the lower
// band of a symmetric D x D system, entry (i, j), i - bw <= j <= i, at Nb[i * (bw + 1) + (j - i + bw)]; fst[i] = the first column of row i that
// can be non-zero (the factor's fill-in stays inside each row's envelope).  Every entry receives its operations in a fixed order, so the
// result is the same bits from call to call and for every MI355_HOST_THREADS; all scratch lives in the call.
#pragma once
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

namespace {
inline int host_threads() {
    static const int n = [] {
        const char* e = getenv("MI355_HOST_THREADS");
        int v = e ? atoi(e) : (int)std::thread::hardware_concurrency();
        if (!e) {
            // several ranks of one node call the alignment at the same moment (the host step is replicated): share the cores between them,
            // a team of spinning threads per rank on oversubscribed cores is what the yield below exists for
            const char* lw = getenv("LOCAL_WORLD_SIZE");
            const int ranks = lw ? atoi(lw) : 1;
            if (ranks > 1) v /= ranks;
        }
        if (v > 32) v = 32;
        return v < 1 ? 1 : v;
    }();
    return n;
}
inline void cpu_relax() {      // a waiting thread must not take issue slots from the hardware thread next to it (it may be the one that works)
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
    __builtin_ia32_pause();
#endif
}
template <class F> void parallel_chunks(size_t n, int threads, F&& f) {          // f(begin, end) on contiguous chunks
    if (threads <= 1 || n < 2) { f((size_t)0, n); return; }
    std::vector<std::thread> th;
    const size_t per = (n + (size_t)threads - 1) / (size_t)threads;
    for (int t = 1; t < threads; t++) { const size_t lo = per * t, hi = lo + per < n ? lo + per : n; if (lo < hi) th.emplace_back([&f, lo, hi] { f(lo, hi); }); }
    f((size_t)0, per < n ? per : n);
    for (auto& x : th) x.join();
}
// Phase (C) of the banded Cholesky below for one row: s[j] -= l_k * pt_k[j] for the panel's columns k in ascending order, j over the row's
// trailing entries.  pt_k = the panel's column k laid out along j (a transposed copy made in phase (B)), so the j loop runs over contiguous
// doubles and the compiler vectorises it; every entry still takes its products one by one in k order, each product rounded, then the
// difference (this file is compiled with -ffp-contract=off): the same bits as the scalar form, for any vector width.  Clones for the
// host's vector unit are picked when the library is loaded (the build machine need not be the machine that runs).
#if defined(__HIP_DEVICE_COMPILE__) || !defined(__x86_64__) || defined(__SANITIZE_THREAD__) || defined(__SANITIZE_ADDRESS__)      // (an ifunc resolver runs before a sanitizer's runtime is up)
#define MI355_SIMD_CLONES
#else
#define MI355_SIMD_CLONES __attribute__((target_clones("avx512f", "avx2", "default")))
#endif
MI355_SIMD_CLONES static void chol_row_update(double* __restrict s, int n, const double* __restrict l, int nk, const double* __restrict pt, size_t pt_stride) {
    // four columns of the panel per walk over the row: an entry is loaded and stored once for four subtractions (one column per walk made the
    // loop memory-bound: C5-sized factorisation 58 -> 38 ms on one thread of the box); per entry the same subtractions in the same order
    int k = 0;
    for (; k + 4 <= nk; k += 4) {
        const double l0 = l[k], l1 = l[k + 1], l2 = l[k + 2], l3 = l[k + 3];
        const double* __restrict p0 = pt + (size_t)k * pt_stride;
        const double* __restrict p1 = p0 + pt_stride;
        const double* __restrict p2 = p1 + pt_stride;
        const double* __restrict p3 = p2 + pt_stride;
        for (int j = 0; j < n; j++) {
            double v = s[j];
            v -= l0 * p0[j]; v -= l1 * p1[j]; v -= l2 * p2[j]; v -= l3 * p3[j];
            s[j] = v;
        }
    }
    for (; k < nk; k++) {
        const double lk = l[k];
        const double* __restrict p = pt + (size_t)k * pt_stride;
        for (int j = 0; j < n; j++) s[j] -= lk * p[j];
    }
}
// Phase (B) for one row below the panel's diagonal block, right-looking: entry j is final once the columns before it have left it, is divided by
// the diagonal, and leaves the row's later entries at once -- s[q] -= L(i, j) * L(j + 1 + q, j), the column of the diagonal block laid out along
// q (dt) -- so the walk is over contiguous doubles; an entry still takes its products one by one in ascending k.  (Columns left of a later
// entry's own envelope contribute products with an exact zero.)
MI355_SIMD_CLONES static void chol_row_forward(double* __restrict r /* entries ja .. jb - 1 of the row */, int n, const double* __restrict diag /* L(j, j) */,
                                               const double* __restrict dt /* dt[j * dts + q] = L(ja + j + 1 + q, ja + j) */, size_t dts, double* __restrict pt /* column of the transposed panel copy */, size_t pts) {
    for (int j = 0; j < n; j++) {
        const double sv = r[j] / diag[j];
        r[j] = sv;
        pt[(size_t)j * pts] = sv;
        const double* __restrict d = dt + (size_t)j * dts;
        double* __restrict s = r + j + 1;
        const int m = n - j - 1;
        for (int q = 0; q < m; q++) s[q] -= sv * d[q];
    }
}

// The envelope of a system with `rows` unknowns per free image: the free images (columns 0 .. nf - 1, in index order) of pair p are
// pair(p, oa, ob) (a negative column = a fixed image).  bw = the half bandwidth in scalar rows, fst as above.
template <class Pair> void envelope_profile(int rows, int nf, size_t n_pairs, Pair&& pair, int& bw, std::vector<int>& fst) {
    int bwb = 0;
    fst.resize((size_t)rows * nf);
    for (int o = 0; o < nf; o++) for (int t = 0; t < rows; t++) fst[rows * o + t] = rows * o;
    for (size_t p = 0; p < n_pairs; p++) {
        int oa, ob;
        pair(p, oa, ob);
        if (oa < 0 || ob < 0 || oa == ob) continue;
        const int hi = oa > ob ? oa : ob, lo = oa > ob ? ob : oa;
        if (hi - lo > bwb) bwb = hi - lo;
        for (int t = 0; t < rows; t++) if (rows * lo < fst[rows * hi + t]) fst[rows * hi + t] = rows * lo;
    }
    bw = rows * bwb + rows - 1;
}

// Cholesky N = L L^T (lower), in place, inside the band, in panels of 64 columns.  Every entry (i, j) still receives the same
// operations in the same order as in the column-by-column form -- N(i, j) minus L(i, k) L(j, k) for ascending k, each product
// subtracted on its own, then the division by the diagonal -- so the factor has the same bits whatever the panel width and the
// number of threads; what changes is who waits for whom: a team walking the columns together met at one barrier per column
// (1497 at C4, 6000 at C5: half of the time), and one dot product per entry is a single dependent chain of subtractions.  Per
// panel: (A) one thread factors the 64 x 64 diagonal block, (B) the rows below it are divided up between the threads, (C) the
// panel's products are subtracted from the trailing band, again by rows, four independent entries at a time.  Three barriers per
// panel.  Returns false when a pivot is not positive (the walk still finishes, so that the team stays in step).
inline bool envelope_cholesky(double* Nb_data, int D, int bw, const std::vector<int>& fst) {
    const size_t W = (size_t)bw + 1;
    double work = 0.0;
    for (int i = 0; i < D; i++) work += (double)(i - fst[i]) * (double)(i - fst[i]);
    // one thread per 2.5e7 multiply-subtracts, up to 16 (measured on the GPU box's host, C5's size, 5e8: 34 ms on one thread, 20 on four, 14 on eight,
    // 12 on sixteen, 11.5 on thirty-two; C4's 3.6e7 stay on one thread: 1.3 ms, starting a team costs about that).  The team scales only since rows
    // keep their owner and eight neighbouring rows share one (see `mine` below): before, two threads took twice as long as one.
    int team = (int)(work / 2.5e7);
    if (team > 16) team = 16;
    if (team > host_threads()) team = host_threads();
    if (team < 1) team = 1;
    constexpr int PW = 64;
    const size_t pts = ((size_t)bw + PW + 7) & ~(size_t)7;       // a panel's columns, transposed: PT[k - p0][i - p1] = L(i, k) for the rows i below the block
    std::vector<double> PT_store((size_t)PW * pts + 8, 0.0), DT((size_t)PW * (PW + 1), 0.0), DG(PW, 1.0);      // DT[(k - p0) * (PW + 1) + (j - k - 1)] = L(j, k) of the diagonal block, j > k
    double* const PT = PT_store.data() + ((64 - (reinterpret_cast<uintptr_t>(PT_store.data()) & 63)) & 63) / sizeof(double);      // on a cache-line boundary: eight rows' entries of a column share a line, and eight rows share an owner
    std::atomic<int> arrived{0}, generation{0}, failed{0};
    auto rowp = [&](int i) -> double* { return Nb_data + (ptrdiff_t)i * (ptrdiff_t)W + (ptrdiff_t)(bw - i); };     // rowp(i)[j] = N(i, j), i - bw <= j <= i
    auto worker = [&](int tid) {
        int gen = 0;
        auto barrier = [&]() {
            if (team <= 1) return;
            gen++;
            if (arrived.fetch_add(1) + 1 == team) { arrived.store(0); generation.store(gen); }
            else { int spins = 0; while (generation.load(std::memory_order_acquire) < gen) { cpu_relax(); if (++spins > 4096) { std::this_thread::yield(); spins = 4000; } } }   // a phase takes microseconds: spin, but yield when the host has fewer cores than threads
        };
        for (int p0 = 0; p0 < D; p0 += PW) {
            const int p1 = p0 + PW < D ? p0 + PW : D;
            if (tid == 0) {                                       // (A) the diagonal block
                for (int j = p0; j < p1; j++) {
                    double* rj = rowp(j);
                    double d = rj[j];
                    for (int k = (fst[j] > p0 ? fst[j] : p0); k < j; k++) d -= rj[k] * rj[k];
                    if (!(d > 0.0)) { failed.store(1); d = 1.0; }        // keep walking so that the team stays in step; the caller sees `failed`
                    d = std::sqrt(d);
                    rj[j] = d;
                    for (int i = j + 1; i < p1 && i <= j + bw; i++) {    // rows of the block that reach column j (half bandwidth below the panel width: adjacent-pair strips)
                        if (fst[i] > j) continue;
                        double* ri = rowp(i);
                        double sv = ri[j];
                        const int ka = fst[i] > fst[j] ? fst[i] : fst[j];
                        for (int k = (ka > p0 ? ka : p0); k < j; k++) sv -= ri[k] * rj[k];
                        ri[j] = sv / d;
                    }
                }
            }
            if (tid == 0) {                                       // the block's columns laid out along the rows (phase B walks them), zeros outside a row's envelope, and its diagonal
                for (int k = p0; k < p1; k++) {
                    DG[k - p0] = rowp(k)[k];
                    for (int j = k + 1; j < p1; j++) DT[(size_t)(k - p0) * (PW + 1) + (size_t)(j - k - 1)] = (fst[j] <= k && j - k <= bw) ? rowp(j)[k] : 0.0;
                }
            }
            barrier();
            const int i_end = p1 - 1 + bw < D - 1 ? p1 - 1 + bw : D - 1;             // last row that holds an entry in a column of the panel
            // rows dealt out one by one: row i of the trailing band has i - p1 + 1 entries to update, contiguous chunks would give the last
            // thread twice the mean
            // rows belong to threads in groups of eight, the same thread in every panel ((i / 8) mod team): a row's entries stay in that core's
            // cache from panel to panel, and the eight doubles of a line of the transposed panel copy have one writer (dealt row by row from the
            // panel's first row on, a row changed hands with every panel and neighbouring rows wrote into the same lines: two threads took twice
            // as long as one)
            auto mine = [&](int i) { return ((i >> 3) % team) == tid; };
            for (int i = p1; i <= i_end; i++) {       // (B) the panel's columns of the rows below the block
                if (!mine(i)) continue;
                double* ri = rowp(i);
                const int j0 = fst[i] > p0 ? fst[i] : p0;
                for (int j = p0; j < j0 && j < p1; j++) PT[(size_t)(j - p0) * pts + (size_t)(i - p1)] = 0.0;      // left of the row's envelope (or the row does not reach the panel at all)
                if (j0 < p1) chol_row_forward(ri + j0, p1 - j0, DG.data() + (j0 - p0), DT.data() + (size_t)(j0 - p0) * (PW + 1), (size_t)PW + 1, PT + (size_t)(j0 - p0) * pts + (size_t)(i - p1), pts);
            }
            barrier();
            // (C) the panel's products leave the trailing band, tile by tile of 64 trailing columns: the tile's part of the transposed panel copy
            // (64 x 64 doubles) stays in the first-level cache while the rows pass (row by row over the whole band it was streamed from the
            // second level once per row: 16 GB at C5)
            constexpr int JT = 64;
            for (int jt = p1; jt <= i_end; jt += JT) {
                for (int i = (jt > p1 ? jt : p1); i <= i_end; i++) {
                    if (!mine(i) || fst[i] >= p1) continue;          // above the tile / the row holds nothing in the panel's columns
                    double* ri = rowp(i);
                    const int k0 = fst[i] > p0 ? fst[i] : p0;
                    const int j0 = fst[i] > p1 ? fst[i] : p1;
                    const int ja = j0 > jt ? j0 : jt, jb = i < jt + JT - 1 ? i : jt + JT - 1;
                    if (ja > jb) continue;
                    // the transposed copy holds L(j, k) for every row j of the trailing band, zeros left of row j's envelope
                    chol_row_update(ri + ja, jb - ja + 1, ri + k0, p1 - k0, PT + (size_t)(k0 - p0) * pts + (size_t)(ja - p1), pts);
                }
            }
            barrier();
        }
    };
    if (team > 1) {
        std::vector<std::thread> th;
        for (int t = 1; t < team; t++) th.emplace_back(worker, t);
        worker(0);
        for (auto& x : th) x.join();
    } else worker(0);
    return failed.load() == 0;
}

// L y = b, L^T x = y in place on the factor envelope_cholesky left; by may be NULL (one right-hand side: the same operations on bx alone)
inline void envelope_solve(const double* Nb_data, int D, int bw, const std::vector<int>& fst, double* bx, double* by) {
    const size_t W = (size_t)bw + 1;
    auto rowp = [&](int i) -> const double* { return Nb_data + (ptrdiff_t)i * (ptrdiff_t)W + (ptrdiff_t)(bw - i); };
    if (!by) {
        for (int i = 0; i < D; i++) {
            const double* ri = rowp(i);
            double sx = bx[i];
            for (int k = fst[i]; k < i; k++) sx -= ri[k] * bx[k];
            bx[i] = sx / ri[i];
        }
        for (int i = D - 1; i >= 0; i--) {
            const double* ri = rowp(i);
            const double xi = bx[i] / ri[i];
            bx[i] = xi;
            for (int k = fst[i]; k < i; k++) bx[k] -= ri[k] * xi;
        }
        return;
    }
    // L y = b, L^T x = y for both right-hand sides in one walk (two independent chains of subtractions; the same operations per side as before)
    for (int i = 0; i < D; i++) {
        const int k0 = fst[i];
        const double* ri = rowp(i);
        double sx = bx[i], sy = by[i];
        for (int k = k0; k < i; k++) { const double l = ri[k]; sx -= l * bx[k]; sy -= l * by[k]; }
        bx[i] = sx / ri[i]; by[i] = sy / ri[i];
    }
    // L^T x = y, row-oriented: once x[i] is final, row i of L (contiguous) takes its products out of the entries above it.  An entry y[k] thus
    // loses L(i, k) x[i] for DESCENDING i -- a fixed order, whatever the thread count.  (Until round 5 the walk went down column i of L for every
    // i: one entry per row of the band, W doubles apart -- 3.3 M cache misses at C5, as long as half the factorisation on 16 threads.)
    for (int i = D - 1; i >= 0; i--) {
        const double* ri = rowp(i);
        const double xi = bx[i] / ri[i], yi = by[i] / ri[i];
        bx[i] = xi; by[i] = yi;
        for (int k = fst[i]; k < i; k++) { const double l = ri[k]; bx[k] -= l * xi; by[k] -= l * yi; }
    }
}
}  // namespace
