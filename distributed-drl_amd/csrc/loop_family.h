// The learner-independent half of the captured learner loops (loop.hip: SAC1 on ddrl_loop_*; dqn_loop.hip: Double-DQN / SQN on
// ddrl_dqn_loop_*): which lengths are captured, which variants of a length a call can reach, and the order in which a call's
// updates are consumed.  Internal to libddrl_hip.so — not part of the C-ABI.
#pragma once
#include "ddrl_common.h"

#include <cstdint>
#include <vector>

namespace ddrl_family {

// One captured length.  exec[pre][start][tail]:
//   pre   0: head-sampled — opens with a stand-alone sampler launch;  1: pre-sampled — the replay before it drew its first batch
//   start the input set of its first update
//   tail  1: the last update draws the first batch of the replay that follows (into the set its own last update does not read)
// INPUT-SET PARITY: both starting sets are captured where a replay can meet them, nothing is tracked across calls.  A
// head-sampled graph starts on set 0 whatever ran before it (its sampler is stream-ordered behind every earlier reader of set 0,
// as the single graph's always was); a pre-sampled graph starts where the replay before it left its draw, which is set 1 only
// behind an odd number of odd-length replays — an odd `per_graph`, the length-1 graph being the last of any call.  Variants
// that no call can reach stay nullptr (variant_needed).
struct Graph { int len; hipGraphExec_t exec[2][2][2]; };

// per_graph, then the powers of two below it, descending
static inline std::vector<Graph> lengths(int per_graph) {
    std::vector<Graph> family;
    family.push_back(Graph{per_graph, {}});
    int p = 1;
    while (p * 2 < per_graph) p *= 2;
    for (; p >= 1 && p < per_graph; p >>= 1) family.push_back(Graph{p, {}});
    return family;
}

// chain: the sampler chain runs across the replays of one call (off: every replay head-sampled on set 0, no tail draw)
static inline bool variant_needed(bool chain, int per_graph, int len, int pre, int start, int tail) {
    if (!chain) return !pre && !start && !tail;
    if (start && (!pre || (per_graph & 1) == 0)) return false;
    if (tail && len == 1 && per_graph != 1) return false;   // the length-1 remainder ends its call
    return true;
}

static inline void destroy(std::vector<Graph> &family) {
    for (auto &g : family)
        for (int v = 0; v < 8; ++v)
            if (g.exec[v >> 2][(v >> 1) & 1][v & 1]) (void)hipGraphExecDestroy(g.exec[v >> 2][(v >> 1) & 1][v & 1]);
    family.clear();
}

// Greedy: per_graph-sized replays, then each power of two at most once (left < per_graph <= 2 x the largest of them).
// The first replay of the call is head-sampled; each replay that another one follows draws that one's first batch.
static inline int replay(const std::vector<Graph> &family, bool chain, int64_t &left, hipStream_t s) {
    bool first = true;
    int set = 0;
    for (const auto &g : family)
        while (left >= g.len) {
            const int pre = (!first && chain) ? 1 : 0, tail = (chain && left > g.len) ? 1 : 0;
            if (!pre) set = 0;
            hipGraphExec_t exec = g.exec[pre][set][tail];
            DDRL_REQUIRE(exec != nullptr, "no captured graph for this replay (internal)");
            DDRL_HIP_CHECK(hipGraphLaunch(exec, s));
            set ^= g.len & 1;
            left -= g.len;
            first = false;
        }
    return DDRL_OK;
}

}  // namespace ddrl_family
