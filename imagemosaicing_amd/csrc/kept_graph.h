// csrc/kept_graph.h -- the connectivity walk the two frame selections share (sharp_solve.cpp: mi355_select_sharp_frames; cover_select.cpp:
// mi355_cover_select): a graph on the frames, from which frames are dropped one at a time, and the question "do the still-kept frames of k's
// component stay connected without k".  Lifted from sharp_solve.cpp, which held it inline.  Host only, no HIP.
#pragma once
#include <cstddef>
#include <utility>
#include <vector>

namespace mi_graph {

struct KeptGraph {
    std::vector<std::vector<int>> part;          // per frame its partners
    std::vector<int> comp, kept_in;              // a frame's component; how many kept frames each component still holds
    std::vector<char> gone;
    std::vector<int> seen, queue;
    int stamp = 0;

    // every frame gets a component (a frame without partners one of its own), found in ascending order of the lowest member
    void build(std::vector<std::vector<int>> partners) {
        part = std::move(partners);
        const int n = (int)part.size();
        comp.assign((size_t)n, -1); kept_in.clear(); gone.assign((size_t)n, 0); seen.assign((size_t)n, -1); stamp = 0;
        for (int s = 0; s < n; s++) {
            if (comp[s] >= 0) continue;
            const int c = (int)kept_in.size();
            queue.assign(1, s); comp[s] = c;
            for (size_t head = 0; head < queue.size(); head++)
                for (int q : part[queue[head]]) if (comp[q] < 0) { comp[q] = c; queue.push_back(q); }
            kept_in.push_back((int)queue.size());
        }
    }
    // how many kept frames a walk from k's first kept partner reaches without passing through k; 0: k has no kept partner
    int reach_without(int k) {
        int start = -1;
        for (int q : part[k]) if (!gone[q]) { start = q; break; }
        if (start < 0) return 0;
        const int i = stamp++;
        int reached = 1;
        queue.assign(1, start); seen[start] = i;
        for (size_t head = 0; head < queue.size(); head++)
            for (int q : part[queue[head]])
                if (q != k && !gone[q] && seen[q] != i) { seen[q] = i; queue.push_back(q); reached++; }
        return reached;
    }
    // the kept frames of k's component other than k (k itself kept)
    int others_kept(int k) const { return kept_in[comp[k]] - 1; }
    void drop(int k) { gone[k] = 1; kept_in[comp[k]]--; }
};

}  // namespace mi_graph
