// csrc/cover_select.cpp -- the host half of cover depth (include/mi355_mosaic.h, "cover depth"): the parameter, order and pair-list checks and
// the selection loop, with one round's statistics behind a callable.  Host-only code, no device work: cover.hip holds the kernel, the
// launcher and the geometry (frame_boxes) and plugs the kernel into this loop (cover.h).
//
//   mi_cover::select     the rule of the header, on boxes.  A round takes the statistics once and walks the waiting candidates in order; a
//                        candidate whose box meets the box of an earlier candidate that still waits, or of one dropped in this round, waits
//                        for the next round, so every settled candidate sees the statistics the sequential greedy would have shown it.  The
//                        connectivity check is sharp_solve.cpp's walk (kept_graph.h) on the pair list restricted to the frames kept on entry.
//   mi355_cover_select   that loop on a survey's geometry with the caller's statistics function.
#include "cover.h"
#include "gain.h"
#include "host_error.h"
#include "kept_graph.h"
#include <algorithm>
#include <cstdint>
#include <vector>

namespace mi_cover {

using mi_gain::check_frames_n;
using mi_gain::check_pairs;
using mi_gain::flat_pairs;

bool check_cover_params(const mi355_cover_params& p, std::string& err) {
    if (p.step < 1 || p.step > 64) { err = "step=" + std::to_string(p.step) + " outside [1, 64]"; return false; }
    if (p.min_depth < 1 || p.min_depth > 8) { err = "min_depth=" + std::to_string(p.min_depth) + " outside [1, 8]"; return false; }
    if (p.max_loss < 0) { err = "max_loss=" + std::to_string(p.max_loss) + " < 0"; return false; }
    return true;
}

namespace {

bool meets(const Box& a, const Box& b) { return a.x0 <= b.x1 && b.x0 <= a.x1 && a.y0 <= b.y1 && b.y0 <= a.y1; }

bool check_order(const int32_t* order, int n_order, int n, std::string& err) {
    std::vector<int> at((size_t)n, -1);
    for (int i = 0; i < n_order; i++) {
        const int k = order[i];
        if (k < 0 || k >= n) { err = "order[" + std::to_string(i) + "]=" + std::to_string(k) + " outside [0, " + std::to_string(n) + ")"; return false; }
        if (at[k] >= 0) { err = "order[" + std::to_string(i) + "]=" + std::to_string(k) + " repeats order[" + std::to_string(at[k]) + "]"; return false; }
        at[k] = i;
    }
    return true;
}

}  // namespace

int select(int n, const Box* box, const char* part, const uint8_t* keep, const int32_t* order, int n_order, const int32_t* pairs_ab, int n_pairs,
           const mi355_cover_params& p, const StatsFn& stats, uint8_t* status, uint8_t* keep_out, int32_t* rounds, int64_t* lost, std::string& err) {
    if (!check_frames_n(n, err) || !check_cover_params(p, err)) return MI355_ERR_ARG;             // before anything is sized by n
    if (!box || !part || !stats || !status || !keep_out || n_pairs < 0 || (n_pairs > 0 && !pairs_ab) || (order && n_order < 0)) { err = "NULL argument or a count < 0"; return MI355_ERR_ARG; }
    if (!check_pairs(flat_pairs(pairs_ab), n_pairs, n, err)) return MI355_ERR_ARG;
    if (order && !check_order(order, n_order, n, err)) return MI355_ERR_ARG;
    std::vector<uint8_t> kept((size_t)n);
    for (int k = 0; k < n; k++) { kept[k] = (part[k] && (!keep || keep[k])) ? 1 : 0; status[k] = MI355_COVER_NOT_CANDIDATE; }
    std::vector<int> waiting, next;
    if (order) {
        for (int i = 0; i < n_order; i++) {
            if (kept[order[i]]) waiting.push_back(order[i]);
            else status[order[i]] = MI355_COVER_NOT_EXAMINED;
        }
    } else {
        for (int k = 0; k < n; k++) if (kept[k]) waiting.push_back(k);
    }
    mi_graph::KeptGraph g;
    const bool graph = n_pairs > 0;
    if (graph) {
        std::vector<std::vector<int>> partners((size_t)n);
        for (int q = 0; q < n_pairs; q++) {
            const int a = pairs_ab[2 * q], b = pairs_ab[2 * q + 1];
            if (kept[a] && kept[b]) { partners[a].push_back(b); partners[b].push_back(a); }
        }
        g.build(std::move(partners));
    }
    std::vector<mi355_cover_frame_stats> fs((size_t)n);
    std::vector<Box> blocked;
    int n_rounds = 0;
    int64_t n_lost = 0;
    const auto crit = [&](int k) { int64_t c = 0; for (int j = 0; j < p.min_depth; j++) c += fs[k].at_depth[j]; return c; };
    while (!waiting.empty()) {
        const int rc = stats(kept.data(), fs.data(), err);
        if (rc != MI355_OK) return rc;
        n_rounds++;
        if (!order && n_rounds == 1)
            std::stable_sort(waiting.begin(), waiting.end(), [&](int x, int y) { return crit(x) < crit(y); });      // ascending crit, lower index first on ties
        blocked.clear(); next.clear();
        for (int k : waiting) {
            bool wait = false;
            for (const Box& b : blocked) if (meets(box[k], b)) { wait = true; break; }
            if (wait) { next.push_back(k); blocked.push_back(box[k]); continue; }
            const int64_t c = crit(k);
            if (c > p.max_loss) status[k] = MI355_COVER_KEPT_COVERAGE;
            else if (graph && g.reach_without(k) != g.others_kept(k)) status[k] = MI355_COVER_CUT_VERTEX;
            else {
                status[k] = MI355_COVER_DROPPED; kept[k] = 0; n_lost += c;
                if (graph) g.drop(k);
                blocked.push_back(box[k]);
            }
        }
        waiting.swap(next);
    }
    std::copy(kept.begin(), kept.end(), keep_out);
    if (rounds) *rounds = n_rounds;
    if (lost) *lost = n_lost;
    return MI355_OK;
}

}  // namespace mi_cover

using namespace mi_cover;

extern "C" void mi355_default_cover_params(mi355_cover_params* p) {
    if (!p) return;
    p->step = 8; p->min_depth = 1; p->max_loss = 0;
}

extern "C" int mi355_cover_select(const int* w, const int* h, int n, const float* h9s, const uint8_t* keep, const int32_t* order, int n_order,
                                  const int32_t* pairs_ab, int n_pairs, const mi355_cover_params* p, mi355_cover_stats_fn stats_fn, void* user,
                                  uint8_t* status, uint8_t* keep_out, int32_t* rounds, int64_t* lost) {
    mi355_cover_params dp;
    if (!p) { mi355_default_cover_params(&dp); p = &dp; }
    std::string err;
    int rc = MI355_ERR_ARG;
    if (!w || !h || !h9s || !stats_fn) err = "NULL argument or a count < 0";
    else if (mi_gain::check_frames_n(n, err)) {                        // before anything is sized by n
        std::vector<Box> box((size_t)n);
        std::vector<char> part((size_t)n);
        rc = frame_boxes(w, h, n, h9s, box.data(), part.data(), err);
        if (rc == MI355_OK)
            rc = select(n, box.data(), part.data(), keep, order, n_order, pairs_ab, n_pairs, *p,
                        [&](const uint8_t* kp, mi355_cover_frame_stats* fs, std::string& e) {
                            const int r = stats_fn(user, kp, fs);
                            if (r != MI355_OK) e = "the statistics function returned " + std::to_string(r);
                            return r;
                        },
                        status, keep_out, rounds, lost, err);
    }
    if (rc != MI355_OK) mi_set_host_error("cover_select: " + err);
    return rc;
}
