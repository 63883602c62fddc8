// csrc/screen.hip -- descriptor-screened pair schedule (gfx950): an exact all-pairs score on the strongest top_k keypoints of every frame,
// then a per-frame nomination of its best partners (include/mi355_mosaic.h, mi355_screen_pairs).  The window schedule of the reference
// (mi355_pair_schedule, MosaicWithoutPos.cpp:5083) matches every pair within `window` frames of capture order, and at C4 97 % of those pairs
// are rejected; a survey whose capture order is not its spatial order (shuffled sets, several flights, the far strip of a lawnmower) has
// no window at all.  The screen proposes the pairs worth matching; mi355_match_pairs(_dev) then matches them unchanged.
//
// Three kernels:
//   screen_topk_kernel    one workgroup per frame: radix select of the top_k keys (response bits, then ~index: response descending,
//                         index ascending -- a total order, so the K-th key is unique), bitonic sort of the survivors in LDS, gather of
//                         their int8 rows and norms into a packed table [n][top_k][128] + [n][top_k].  Padding rows are zeros with the
//                         norm SENTINEL (2^28): their distance to any query exceeds every real one (<= 128 * 255^2 < 2^23), so they are
//                         never a nearest neighbour, and a second-nearest distance >= 2^27 reads as +infinity.
//   screen_pairs_kernel   one workgroup per candidate pair (a, b): both frames' rows in LDS (pitch 144 B, the matcher's bank-conflict-free
//                         staging), v_mfma_i32_32x32x32_i8 in the matcher's orientation (match.hip: the TRAIN tile is the A operand, the QUERY
//                         tile the B operand, so every lane holds 16 train rows of ONE query and the running (best, d1, d2) is lane-local).
//                         The other direction runs as a second pass with the roles swapped: twice the MFMAs, but no cross-lane reduction
//                         of 16 accumulators per tile (a 32-lane min/argmin of 16 registers costs 5 shuffles + 3 VALU each, ~30 VALU per
//                         element against the 6 of the lane-local update).  The cross-lane variant was not built and measured; the
//                         estimate above is why this one was written first.  Candidate pairs are a flat list in (a, b) order placed with
//                         match.hip's xcd_owned, so the pairs of one frame a run under one L2.
//   screen_select_kernel  per row a: a histogram of its in-scope scores (<= 513 bins) gives the threshold score and, by an ordered scan of the
//                         ties, the last position nominated; then every kept pair (a nominates b or b nominates a) of the rows this rank owns
//                         is counted and written in (a, b) order.
//
// The score is exact (tests/screen_ref.py restates it in numpy): D(q, t) = |q'|^2 + |t'|^2 - 2 q'.t' on the shifted int8 rows is |q - t|^2
// on the u8 descriptors; nn(q) = argmin over the other frame's list (ties: lower position), d2 the second smallest over the multiset;
// score = #q with nn(nn(q)) == q and both passing 10000 d1 < ratio_pct^2 d2 (int64; skipped at ratio_pct == 100).
#include "common.h"
#include <algorithm>
#include <unordered_map>

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr int SCREEN_MAX_K = 512;
constexpr int SCREEN_MAX_N = 16384;
constexpr int SENTINEL = 1 << 28;          // norm of a padding row
constexpr int INF_D = 1 << 27;             // a distance at or above this is +infinity (it involves a padding row)
constexpr int PITCH = 128 + 16;            // LDS bytes per staged row
constexpr int TOPK_NT = 512;
constexpr int PAIR_NT = 256;
constexpr int SEL_NT = 256;
constexpr long long PAIR_CHUNK = 1ll << 22; // workgroups per launch of screen_pairs_kernel (grid x threads stays below 2^32)

struct TopkFrame { const mi355_keypoint* kp; const int8_t* s8; const int* n8; int n; int _pad; };

__device__ __forceinline__ int xcd_owned(int bid, int nb) {       // match.hip: XCD x owns a contiguous eighth of the list
    const int q = nb >> 3, r = nb & 7, xcd = bid & 7, local = bid >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + local;
}

__device__ __forceinline__ int med3_i32(int a, int b, int c) { int r; asm("v_med3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }

// the ordering key of keypoint i: response descending (as a number: -0 == +0), then index ascending; all keys are distinct and >= 2^31
__device__ __forceinline__ unsigned long long topk_key(const mi355_keypoint* kp, int i) {
    unsigned u = __float_as_uint(kp[i].response);
    if (u == 0x80000000u) u = 0u;
    const unsigned m = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)m << 32) | (unsigned long long)(~(unsigned)i);
}

__global__ __launch_bounds__(TOPK_NT) void screen_topk_kernel(const TopkFrame* frames, int K, int8_t* tab, int* tnorm, int* tcnt) {
    __shared__ unsigned hist[256];
    __shared__ unsigned long long s_keys[SCREEN_MAX_K];
    __shared__ unsigned long long s_prefix, s_mask;
    __shared__ int s_krem, s_cnt;
    const TopkFrame f = frames[blockIdx.x];
    const int tid = threadIdx.x, n = f.n, m = n < K ? n : K;
    unsigned long long thr = 0;                               // keys >= thr survive
    if (n > K) {
        if (tid == 0) { s_prefix = 0; s_mask = 0; s_krem = K; }
        for (int shift = 56; shift >= 0; shift -= 8) {
            for (int d = tid; d < 256; d += TOPK_NT) hist[d] = 0;
            __syncthreads();
            const unsigned long long prefix = s_prefix, mask = s_mask;
            for (int i = tid; i < n; i += TOPK_NT) {
                const unsigned long long key = topk_key(f.kp, i);
                if ((key & mask) == prefix) atomicAdd(&hist[(unsigned)(key >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                int krem = s_krem, d = 255;
                for (; d > 0; d--) { const int c = (int)hist[d]; if (krem <= c) break; krem -= c; }
                s_krem = krem;
                s_prefix = prefix | ((unsigned long long)d << shift);
                s_mask = mask | (255ull << shift);
            }
            __syncthreads();
        }
        thr = s_prefix;                                       // the K-th largest key itself
    }
    if (tid == 0) s_cnt = 0;
    for (int i = tid; i < SCREEN_MAX_K; i += TOPK_NT) s_keys[i] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += TOPK_NT) {
        const unsigned long long key = topk_key(f.kp, i);
        if (key >= thr) { const int slot = atomicAdd(&s_cnt, 1); if (slot < SCREEN_MAX_K) s_keys[slot] = key; }
    }
    __syncthreads();
    int P = 32; while (P < K) P <<= 1;                        // bitonic, descending (the zero padding keys go last)
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += TOPK_NT) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const unsigned long long a = s_keys[i], b = s_keys[ixj];
                    const bool desc = (i & k) == 0;
                    if ((a < b) == desc) { s_keys[i] = b; s_keys[ixj] = a; }
                }
            }
            __syncthreads();
        }
    int8_t* trow = tab + (size_t)blockIdx.x * K * 128;
    for (int c = tid; c < K * 8; c += TOPK_NT) {              // 16 B per thread and step
        const int p = c >> 3, part = c & 7;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (p < m) {
            const int idx = (int)(~(unsigned)(s_keys[p] & 0xffffffffull));
            v = *reinterpret_cast<const uint4*>(f.s8 + (size_t)idx * 128 + part * 16);
        }
        *reinterpret_cast<uint4*>(trow + (size_t)p * 128 + part * 16) = v;
    }
    for (int p = tid; p < K; p += TOPK_NT) {
        int nv = SENTINEL;
        if (p < m) nv = f.n8[(int)(~(unsigned)(s_keys[p] & 0xffffffffull))];
        tnorm[(size_t)blockIdx.x * K + p] = nv;
    }
    if (tid == 0) tcnt[blockIdx.x] = m;
}

// Nearest neighbours of the rows of Q among the rows of T, both in LDS.  res[q] = 2 nn(q) + (q passes the ratio test), or -1 (no row in T).
__device__ __forceinline__ void nn_direction(const int8_t* sQ, const int* nQ, int mq, const int8_t* sT, const int* nT, int mt, int ratio_pct, int* res) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hi = lane >> 5, col = lane & 31;
    const int qblocks = (mq + 31) >> 5, tblocks = (mt + 31) >> 5;
    for (int qb = wave; qb < qblocks; qb += PAIR_NT / 64) {
        i32x4 bq[4];
#pragma unroll
        for (int ks = 0; ks < 4; ks++) bq[ks] = *reinterpret_cast<const i32x4*>(sQ + (qb * 32 + col) * PITCH + ks * 32 + hi * 16);
        int d1 = 0x7fffffff, d2 = 0x7fffffff, i1 = -1;       // over x = |t'|^2 - 2 q'.t' (the query's norm is added at the end)
        for (int tb = 0; tb < tblocks; tb++) {
            i32x4 fa[4];
#pragma unroll
            for (int ks = 0; ks < 4; ks++) fa[ks] = *reinterpret_cast<const i32x4*>(sT + (tb * 32 + col) * PITCH + ks * 32 + hi * 16);
            i32x16 acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[0], bq[0], i32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, 0, 0, 0);
#pragma unroll
            for (int ks = 1; ks < 4; ks++) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[ks], bq[ks], acc, 0, 0, 0);
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const i32x4 nt = *reinterpret_cast<const i32x4*>(nT + tb * 32 + 8 * g + 4 * hi);   // C/D layout: rows 8g + 4hi + r in acc[4g + r]
                const int ntv[4] = {nt.x, nt.y, nt.z, nt.w};
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int x = ntv[r] - 2 * acc[4 * g + r];
                    const int row = tb * 32 + 8 * g + 4 * hi + r;   // ascending within the lane: a strict < keeps the lower position
                    d2 = med3_i32(d1, d2, x);
                    i1 = x < d1 ? row : i1;
                    d1 = min(d1, x);
                }
            }
        }
        // merge the two half-waves (same query, disjoint rows); ties -> lower position; d2 over the union multiset
        const int o1 = __shfl_xor(d1, 32), o2 = __shfl_xor(d2, 32), oi = __shfl_xor(i1, 32);
        const bool other = o1 < d1 || (o1 == d1 && oi >= 0 && (i1 < 0 || oi < i1));
        const int b1 = other ? o1 : d1, bi = other ? oi : i1;
        const int b2 = min(min(d2, o2), max(d1, o1));
        const int q = qb * 32 + col;
        if (hi == 0 && q < mq) {
            int r = -1;
            if (bi >= 0 && bi < mt) {
                const int nq = nQ[q];
                const long long dd1 = (long long)b1 + nq, dd2 = (long long)b2 + nq;
                const bool pass = ratio_pct >= 100 || dd2 >= INF_D || 10000ll * dd1 < (long long)ratio_pct * ratio_pct * dd2;
                r = 2 * bi + (pass ? 1 : 0);
            }
            res[q] = r;
        }
    }
}

__global__ __launch_bounds__(PAIR_NT) void screen_pairs_kernel(const int8_t* tab, const int* tnorm, const int* tcnt, const long long* rowoff, int n,
                                                                long long base, int K, int ratio_pct, int* scores) {
    extern __shared__ __attribute__((aligned(16))) int8_t lds[];
    int8_t* sA = lds;
    int8_t* sB = lds + (size_t)K * PITCH;
    int* nA = reinterpret_cast<int*>(lds + (size_t)2 * K * PITCH);
    int* nB = nA + K;
    int* rA = nB + K;
    int* rB = rA + K;
    int* s_cnt = rB + K;
    const long long g = base + xcd_owned(blockIdx.x, gridDim.x);
    int lo = 0, hi_ = n - 1;                                  // the row a: the largest a with rowoff[a] <= g
    while (lo < hi_) { const int mid = (lo + hi_ + 1) >> 1; if (rowoff[mid] <= g) lo = mid; else hi_ = mid - 1; }
    const int a = lo, b = a + 1 + (int)(g - rowoff[a]);
    const int tid = threadIdx.x;
    const int ma = tcnt[a], mb = tcnt[b];
    if (ma == 0 || mb == 0) {                                 // an empty frame scores 0
        if (tid == 0) { scores[(size_t)a * n + b] = 0; scores[(size_t)b * n + a] = 0; }
        return;
    }
    const int ra = (ma + 31) & ~31, rb = (mb + 31) & ~31;     // rows past m up to the block edge are the table's padding rows
    const int8_t* ta = tab + (size_t)a * K * 128;
    const int8_t* tb = tab + (size_t)b * K * 128;
    for (int c = tid; c < ra * 8; c += PAIR_NT) *reinterpret_cast<uint4*>(sA + (c >> 3) * PITCH + (c & 7) * 16) = *reinterpret_cast<const uint4*>(ta + (size_t)c * 16);
    for (int c = tid; c < rb * 8; c += PAIR_NT) *reinterpret_cast<uint4*>(sB + (c >> 3) * PITCH + (c & 7) * 16) = *reinterpret_cast<const uint4*>(tb + (size_t)c * 16);
    for (int i = tid; i < ra; i += PAIR_NT) nA[i] = tnorm[(size_t)a * K + i];
    for (int i = tid; i < rb; i += PAIR_NT) nB[i] = tnorm[(size_t)b * K + i];
    if (tid == 0) *s_cnt = 0;
    __syncthreads();
    nn_direction(sA, nA, ma, sB, nB, mb, ratio_pct, rA);
    nn_direction(sB, nB, mb, sA, nA, ma, ratio_pct, rB);
    __syncthreads();
    int cnt = 0;
    for (int q = tid; q < ma; q += PAIR_NT) {
        const int r = rA[q];
        if (r < 0 || !(r & 1)) continue;
        const int rr = rB[r >> 1];
        if (rr >= 0 && (rr & 1) && (rr >> 1) == q) cnt++;
    }
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if ((tid & 63) == 0 && cnt) atomicAdd(s_cnt, cnt);
    __syncthreads();
    if (tid == 0) { scores[(size_t)a * n + b] = *s_cnt; scores[(size_t)b * n + a] = *s_cnt; }
}

// block-wide exclusive prefix of a flag in (thread) order; returns the total
__device__ __forceinline__ int block_prefix(bool flag, int* s_wave, int& before) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long m = __ballot(flag);
    if (lane == 0) s_wave[wave] = __popcll(m);
    __syncthreads();
    int off = 0, total = 0;
    for (int w = 0; w < SEL_NT / 64; w++) { const int c = s_wave[w]; if (w < wave) off += c; total += c; }
    before = off + __popcll(m & ((1ull << lane) - 1ull));
    __syncthreads();
    return total;
}

// phase 0: per row the nomination threshold thr[a] and the last tied position cut[a] (a nominates b iff s > thr, or s == thr and b <= cut);
// phase 1: per owned row the count of kept pairs (a, b > a); phase 2: those pairs written at off[a] in b order
template <int PHASE>
__global__ __launch_bounds__(SEL_NT) void screen_select_kernel(const int* scores, int n, int window, int partners, int min_score, int K,
                                                               int* thr, int* cut, int rank, int world, const long long* off, int* cnt,
                                                               int32_t* out_ab, int32_t* out_s) {
    __shared__ int hist[SCREEN_MAX_K + 1];
    __shared__ int s_wave[SEL_NT / 64];
    __shared__ int s_thr, s_need, s_cut;
    const int a = blockIdx.x, tid = threadIdx.x;
    const int* row = scores + (size_t)a * n;
    const int emin = min_score > 0 ? min_score : 0;
    if (PHASE == 0) {
        const int b0 = window > 0 ? max(0, a - window + 1) : 0, b1 = window > 0 ? min(n, a + window) : n;
        if (partners == 0) { if (tid == 0) { thr[a] = emin - 1; cut[a] = -1; } return; }
        for (int s = tid; s <= K; s += SEL_NT) hist[s] = 0;
        __syncthreads();
        for (int b = b0 + tid; b < b1; b += SEL_NT) { const int s = row[b]; if (s >= emin && s <= K) atomicAdd(&hist[s], 1); }
        __syncthreads();
        if (tid == 0) {
            int cum = 0, t = emin - 1, need = 0;
            for (int s = K; s >= emin; s--) { if (cum + hist[s] >= partners) { t = s; need = partners - cum; break; } cum += hist[s]; }
            s_thr = t; s_need = need; s_cut = -1;
        }
        __syncthreads();
        const int t = s_thr;
        int need = s_need;
        if (need > 0) {                                          // the need-th position (ascending) whose score equals t
            for (int c0 = b0; c0 < b1; c0 += SEL_NT) {           // uniform trip count: every thread reaches the barriers
                const int b = c0 + tid;
                const bool f = b < b1 && row[b] == t;
                int before = 0;
                const int tot = block_prefix(f, s_wave, before);
                if (f && before == need - 1) s_cut = b;
                need -= tot;
                if (need <= 0) break;
            }
        }
        __syncthreads();
        if (tid == 0) { thr[a] = t; cut[a] = s_cut; }
        return;
    }
    if (a % world != rank) { if (PHASE == 1 && tid == 0) cnt[a] = 0; return; }
    const int bend = window > 0 ? min(n, a + window) : n;
    const int ta = thr[a], ca = cut[a];
    long long pos = PHASE == 2 ? off[a] : 0;
    int total = 0;
    for (int c0 = a + 1; c0 < bend; c0 += SEL_NT) {
        const int b = c0 + tid;
        bool keep = false;
        int s = -1;
        if (b < bend) {
            s = row[b];
            if (s >= emin) {
                const int tb = thr[b], cb = cut[b];
                keep = s > ta || (s == ta && b <= ca) || s > tb || (s == tb && a <= cb);
            }
        }
        int before = 0;
        const int tot = block_prefix(keep, s_wave, before);
        if (PHASE == 2 && keep) {
            const long long o = pos + before;
            out_ab[2 * o] = a; out_ab[2 * o + 1] = b; out_s[o] = s;
        }
        pos += tot; total += tot;
    }
    if (PHASE == 1 && tid == 0) cnt[a] = total;
}

size_t pairs_lds_bytes(int K) { return (size_t)2 * K * PITCH + (size_t)4 * K * sizeof(int) + 16; }

int check_params(mi355_ctx* ctx, const mi355_screen_params* p, int n) {
    if (n < 0 || n > SCREEN_MAX_N) { ctx->set_error("screen: n=" + std::to_string(n) + " must be in [0, " + std::to_string(SCREEN_MAX_N) + "]"); return MI355_ERR_ARG; }
    if (p->top_k < 32 || p->top_k > SCREEN_MAX_K || p->top_k % 32 != 0) { ctx->set_error("screen: top_k=" + std::to_string(p->top_k) + " must be a multiple of 32 in [32, 512]"); return MI355_ERR_ARG; }
    if (p->partners < 0) { ctx->set_error("screen: partners=" + std::to_string(p->partners) + " must be >= 0"); return MI355_ERR_ARG; }
    if (p->ratio_pct < 1 || p->ratio_pct > 100) { ctx->set_error("screen: ratio_pct=" + std::to_string(p->ratio_pct) + " must be in [1, 100]"); return MI355_ERR_ARG; }
    if (p->window == 1 || p->window < 0) { ctx->set_error("screen: window=" + std::to_string(p->window) + " must be 0 (all pairs) or >= 2"); return MI355_ERR_ARG; }
    return MI355_OK;
}

// the scores of every in-scope pair into d_scores (n x n, -1 elsewhere); ctx lock held, parameters checked
int screen_scores(mi355_ctx* ctx, const int32_t* img_ids, int n, const mi355_screen_params* p, int32_t* d_scores) {
    if (n > 0 && !img_ids) { ctx->set_error("screen: img_ids is NULL"); return MI355_ERR_ARG; }
    {
        std::unordered_map<int, int> seen;
        for (int k = 0; k < n; k++) {
            auto r = seen.emplace(img_ids[k], k);
            if (!r.second) { ctx->set_error("screen: duplicate img_id " + std::to_string(img_ids[k]) + " at positions " + std::to_string(r.first->second) + " and " + std::to_string(k)); return MI355_ERR_ARG; }
        }
    }
    if (n == 0) return MI355_OK;
    for (int k = 0; k < n; k++)
        if (ctx->feats.find(img_ids[k]) == ctx->feats.end()) { ctx->set_error("screen: img_id " + std::to_string(img_ids[k]) + " (position " + std::to_string(k) + ") has no resident SIFT features"); return MI355_ERR_ARG; }
    { int rc = mi_resolve_features_of(ctx, img_ids, n); if (rc != MI355_OK) return rc; }
    const int K = p->top_k;
    std::vector<TopkFrame> fr(n);
    for (int k = 0; k < n; k++) {
        const Features& f = ctx->feats[img_ids[k]];
        if (f.n > 0 && (f.npad < f.n || !f.kp.p || !f.s8.p || !f.n8.p)) { ctx->set_error("screen: the matcher's operands of image " + std::to_string(img_ids[k]) + " are incomplete"); return MI355_ERR_ARG; }
        fr[k].kp = f.kp.as<mi355_keypoint>(); fr[k].s8 = f.s8.as<int8_t>(); fr[k].n8 = f.n8.as<int>(); fr[k].n = f.n; fr[k]._pad = 0;
    }
    const int win = p->window > 0 ? p->window : n;
    std::vector<long long> rowoff((size_t)n + 1, 0);
    for (int a = 0; a < n; a++) { const int c = std::min(n - 1 - a, win - 1); rowoff[a + 1] = rowoff[a] + (c > 0 ? c : 0); }
    const long long total = rowoff[n];
    DevBuf& dfr = ctx->buf("screen_frames"); DevBuf& dtab = ctx->buf("screen_tab"); DevBuf& dnorm = ctx->buf("screen_tnorm");
    DevBuf& dcnt = ctx->buf("screen_tcnt"); DevBuf& droff = ctx->buf("screen_rowoff");
    MI_HIP(dfr.reserve(sizeof(TopkFrame) * n));
    MI_HIP(dtab.reserve((size_t)n * K * 128));
    MI_HIP(dnorm.reserve((size_t)n * K * sizeof(int)));
    MI_HIP(dcnt.reserve((size_t)n * sizeof(int)));
    MI_HIP(droff.reserve(((size_t)n + 1) * sizeof(long long)));
    MI_HIP(hipMemcpyAsync(dfr.p, fr.data(), sizeof(TopkFrame) * n, hipMemcpyHostToDevice, ctx->stream));
    MI_HIP(hipMemcpyAsync(droff.p, rowoff.data(), ((size_t)n + 1) * sizeof(long long), hipMemcpyHostToDevice, ctx->stream));
    MI_HIP(hipMemsetAsync(d_scores, 0xff, (size_t)n * n * sizeof(int32_t), ctx->stream));
    {
        ProfScope ps(ctx, "screen_topk", (double)n * K * 132.0);
        hipLaunchKernelGGL(screen_topk_kernel, dim3(n), dim3(TOPK_NT), 0, ctx->stream, dfr.as<TopkFrame>(), K, dtab.as<int8_t>(), dnorm.as<int>(), dcnt.as<int>());
        MI_HIP(hipGetLastError());
    }
    if (total > 0) {
        const size_t lds = pairs_lds_bytes(K);
        MI_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(screen_pairs_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        ProfScope ps(ctx, "screen_pairs", (double)total * 2.0 * K * 132.0);
        for (long long base = 0; base < total; base += PAIR_CHUNK) {
            const long long cnt = std::min(PAIR_CHUNK, total - base);
            hipLaunchKernelGGL(screen_pairs_kernel, dim3((unsigned)cnt), dim3(PAIR_NT), lds, ctx->stream, dtab.as<int8_t>(), dnorm.as<int>(), dcnt.as<int>(),
                               droff.as<long long>(), n, base, K, p->ratio_pct, d_scores);
            MI_HIP(hipGetLastError());
        }
    }
    MI_HIP(hipStreamSynchronize(ctx->stream));               // the host tables above are locals
    return MI355_OK;
}

}  // namespace

extern "C" void mi355_default_screen_params(mi355_screen_params* p) {
    if (!p) return;
    p->top_k = 256; p->partners = MI355_SCREEN_DEFAULT_PARTNERS; p->min_score = MI355_SCREEN_DEFAULT_MIN_SCORE; p->ratio_pct = 80; p->window = 0;
}

extern "C" int mi355_screen_scores_dev(mi355_ctx* ctx, const int32_t* img_ids, int n, const mi355_screen_params* p, int32_t* d_scores) {
    LOCKED_PROLOGUE
    mi355_screen_params dp;
    if (!p) { mi355_default_screen_params(&dp); p = &dp; }
    { int rc = check_params(ctx, p, n); if (rc != MI355_OK) return rc; }
    if (n > 0 && !d_scores) { ctx->set_error("screen_scores_dev: d_scores is NULL"); return MI355_ERR_ARG; }
    return screen_scores(ctx, img_ids, n, p, d_scores);
}

extern "C" int mi355_screen_pairs(mi355_ctx* ctx, const int32_t* img_ids, int n, const mi355_screen_params* p, int rank, int world,
                                  int32_t* pairs_ij, int32_t* scores, int max_pairs, int* n_pairs) {
    LOCKED_PROLOGUE
    mi355_screen_params dp;
    if (!p) { mi355_default_screen_params(&dp); p = &dp; }
    { int rc = check_params(ctx, p, n); if (rc != MI355_OK) return rc; }
    if (world < 1 || rank < 0 || rank >= world) { ctx->set_error("screen_pairs: rank=" + std::to_string(rank) + " / world=" + std::to_string(world) + " (need world >= 1, 0 <= rank < world)"); return MI355_ERR_ARG; }
    if (!n_pairs) { ctx->set_error("screen_pairs: n_pairs is NULL"); return MI355_ERR_ARG; }
    if (max_pairs < 0) { ctx->set_error("screen_pairs: max_pairs=" + std::to_string(max_pairs) + " must be >= 0"); return MI355_ERR_ARG; }
    *n_pairs = 0;
    DevBuf& dsc = ctx->buf("screen_scores");
    MI_HIP(dsc.reserve((size_t)(n > 0 ? n : 1) * (n > 0 ? n : 1) * sizeof(int32_t)));
    { int rc = screen_scores(ctx, img_ids, n, p, dsc.as<int32_t>()); if (rc != MI355_OK) return rc; }
    if (n < 2) return MI355_OK;
    const int K = p->top_k;
    DevBuf& dthr = ctx->buf("screen_thr"); DevBuf& dcut = ctx->buf("screen_cut"); DevBuf& drc = ctx->buf("screen_rowcnt"); DevBuf& doff = ctx->buf("screen_off");
    MI_HIP(dthr.reserve((size_t)n * sizeof(int))); MI_HIP(dcut.reserve((size_t)n * sizeof(int)));
    MI_HIP(drc.reserve((size_t)n * sizeof(int))); MI_HIP(doff.reserve((size_t)n * sizeof(long long)));
    {
        ProfScope ps(ctx, "screen_select", (double)n * n * 8.0);
        hipLaunchKernelGGL(screen_select_kernel<0>, dim3(n), dim3(SEL_NT), 0, ctx->stream, dsc.as<int>(), n, p->window, p->partners, p->min_score, K,
                           dthr.as<int>(), dcut.as<int>(), rank, world, (const long long*)nullptr, (int*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr);
        hipLaunchKernelGGL(screen_select_kernel<1>, dim3(n), dim3(SEL_NT), 0, ctx->stream, dsc.as<int>(), n, p->window, p->partners, p->min_score, K,
                           dthr.as<int>(), dcut.as<int>(), rank, world, (const long long*)nullptr, drc.as<int>(), (int32_t*)nullptr, (int32_t*)nullptr);
        MI_HIP(hipGetLastError());
    }
    std::vector<int> rc_h(n);
    MI_HIP(hipMemcpyAsync(rc_h.data(), drc.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    MI_HIP(hipStreamSynchronize(ctx->stream));
    std::vector<long long> off(n);
    long long tot = 0;
    for (int a = 0; a < n; a++) { off[a] = tot; tot += rc_h[a]; }
    if (tot > 0x7fffffffll) { ctx->set_error("screen_pairs: " + std::to_string(tot) + " pairs do not fit an int count"); return MI355_ERR_ARG; }
    *n_pairs = (int)tot;
    if (!pairs_ij && !scores) return MI355_OK;                 // count only
    if (tot == 0) return MI355_OK;
    DevBuf& dab = ctx->buf("screen_ab"); DevBuf& ds = ctx->buf("screen_s");
    MI_HIP(dab.reserve((size_t)tot * 2 * sizeof(int32_t))); MI_HIP(ds.reserve((size_t)tot * sizeof(int32_t)));
    MI_HIP(hipMemcpyAsync(doff.p, off.data(), (size_t)n * sizeof(long long), hipMemcpyHostToDevice, ctx->stream));
    {
        ProfScope ps(ctx, "screen_select", (double)n * n * 8.0);
        hipLaunchKernelGGL(screen_select_kernel<2>, dim3(n), dim3(SEL_NT), 0, ctx->stream, dsc.as<int>(), n, p->window, p->partners, p->min_score, K,
                           dthr.as<int>(), dcut.as<int>(), rank, world, doff.as<long long>(), (int*)nullptr, dab.as<int32_t>(), ds.as<int32_t>());
        MI_HIP(hipGetLastError());
    }
    const long long keep = std::min<long long>(tot, max_pairs);
    std::vector<int32_t> ab((size_t)keep * 2 + 2), sc((size_t)keep + 1);
    if (keep > 0) {
        MI_HIP(hipMemcpyAsync(ab.data(), dab.p, (size_t)keep * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        MI_HIP(hipMemcpyAsync(sc.data(), ds.p, (size_t)keep * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    MI_HIP(hipStreamSynchronize(ctx->stream));
    for (long long k = 0; k < keep; k++) {
        if (pairs_ij) { pairs_ij[2 * k] = img_ids[ab[2 * k]]; pairs_ij[2 * k + 1] = img_ids[ab[2 * k + 1]]; }
        if (scores) scores[k] = sc[k];
    }
    if (tot > max_pairs) { ctx->set_error("screen_pairs: " + std::to_string(tot) + " pairs, max_pairs=" + std::to_string(max_pairs)); return MI355_ERR_ARG; }
    return MI355_OK;
}
