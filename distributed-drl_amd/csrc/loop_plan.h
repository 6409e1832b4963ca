// The pure decisions of the captured learner loops (loop_family.h): which lengths are captured, which variants of a length a
// call can reach, and the order in which a call's updates are consumed.  No HIP here: tests/test_loop_plan_cpu.py compiles this
// header with the host compiler and walks every plan.  Internal to libddrl_hip.so — not part of the C-ABI.
#pragma once
#include <cstdint>
#include <vector>

namespace ddrl_plan {

// per_graph, then the powers of two below it, descending
static inline std::vector<int> lengths(int per_graph) {
    std::vector<int> lens{per_graph};
    int p = 1;
    while (p * 2 < per_graph) p *= 2;
    for (; p >= 1 && p < per_graph; p >>= 1) lens.push_back(p);
    return lens;
}

// Variant (pre, start, tail) of a captured length:
//   pre   0: head-sampled — opens with a stand-alone sampler launch;  1: pre-sampled — the replay before it drew its first batch
//   start the input set of its first update
//   tail  1: the last update draws the first batch of the replay that follows (into the set its own last update does not read)
// INPUT-SET PARITY: both starting sets are captured where a replay can meet them, nothing is tracked across calls.  A
// head-sampled graph starts on set 0 whatever ran before it (its sampler is stream-ordered behind every earlier reader of set 0,
// as the single graph's always was); a pre-sampled graph starts where the replay before it left its draw, which is set 1 only
// behind an odd number of odd-length replays — an odd `per_graph`, the length-1 graph being the last of any call.  Variants
// that no call can reach are not captured.
static inline bool variant_needed(int per_graph, int len, int pre, int start, int tail) {
    if (start && (!pre || (per_graph & 1) == 0)) return false;
    if (tail && len == 1 && per_graph != 1) return false;   // the length-1 remainder ends its call
    return true;
}

struct Step { int index, pre, start, tail; };   // index into lengths(per_graph); the variant to replay

// A call of n updates.  Greedy: per_graph-sized replays, then each power of two at most once (what is left is < per_graph <= 2 x
// the largest of them).  The first replay of the call is head-sampled; each replay that another one follows draws that one's
// first batch.
static inline std::vector<Step> plan(int per_graph, int64_t n) {
    const std::vector<int> lens = lengths(per_graph);
    std::vector<Step> steps;
    int set = 0;
    for (int k = 0; k < (int)lens.size(); ++k)
        for (; n >= lens[k]; n -= lens[k]) {
            steps.push_back(Step{k, steps.empty() ? 0 : 1, set, n > lens[k] ? 1 : 0});
            set ^= lens[k] & 1;
        }
    return steps;
}

}  // namespace ddrl_plan
