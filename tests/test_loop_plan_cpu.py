"""csrc/loop_plan.h: the pure decisions of the captured learner loops (ddrl_loop_run, ddrl_dqn_loop_run) — which lengths are
captured, which variants of a length exist, and which variant each replay of a call of n updates launches.  The header includes no
HIP header, so a small driver is compiled against it with the host C++ compiler and its output checked for every graph size in
1 .. 64 plus 4095 and 4096 and every call length in 0 .. 3 x size + 5.  A step outside the variant table is the loop's
"no captured graph for this replay (internal)" error."""
import os
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "distributed-drl_amd", "csrc")
SIZES = list(range(1, 65)) + [4095, 4096]

# One line per size with its lengths, one per length with the 8 variant_needed bits (v = pre * 4 + start * 2 + tail), one per
# call length with its steps coded as index * 8 + v.
DRIVER = r"""
#include "loop_plan.h"
#include <cstdio>
#include <cstdlib>
int main(int argc, char **argv) {
    for (int a = 1; a < argc; ++a) {
        const int pg = atoi(argv[a]);
        const std::vector<int> lens = ddrl_plan::lengths(pg);
        printf("L %d", pg);
        for (int len : lens) printf(" %d", len);
        printf("\n");
        for (int len : lens) {
            printf("V %d %d", pg, len);
            for (int v = 0; v < 8; ++v) printf(" %d", ddrl_plan::variant_needed(pg, len, v >> 2, (v >> 1) & 1, v & 1) ? 1 : 0);
            printf("\n");
        }
        for (long long n = 0; n <= 3LL * pg + 5; ++n) {
            printf("P %d %lld", pg, n);
            for (const ddrl_plan::Step &s : ddrl_plan::plan(pg, n)) {
                if (s.index < 0 || s.index >= (int)lens.size() || (s.pre | s.start | s.tail) >> 1) return 2;
                printf(" %d", s.index * 8 + s.pre * 4 + s.start * 2 + s.tail);
            }
            printf("\n");
        }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler on PATH")
    tmp = tmp_path_factory.mktemp("loop_plan")
    src, exe = str(tmp / "plan_driver.cpp"), str(tmp / "plan_driver")
    with open(src, "w") as f:
        f.write(DRIVER)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe])
    out = subprocess.check_output([exe] + [str(p) for p in SIZES], text=True)
    lengths, needed, steps = {}, {}, {}
    for line in out.splitlines():
        kind, pg, *rest = line.split()
        pg, rest = int(pg), [int(x) for x in rest]
        if kind == "L":
            lengths[pg] = rest
        elif kind == "V":
            needed[pg, rest[0]] = rest[1:]
        else:
            steps[pg, rest[0]] = [(c >> 3, (c >> 2) & 1, (c >> 1) & 1, c & 1) for c in rest[1:]]
    return lengths, needed, steps


def test_lengths_are_the_size_and_the_powers_of_two_below_it(plans):
    lengths = plans[0]
    assert sorted(lengths) == SIZES
    for pg in SIZES:
        want = [pg] + [1 << k for k in range(12, -1, -1) if (1 << k) < pg]
        assert lengths[pg] == want, pg


def test_every_call_is_covered_in_order_by_reachable_variants(plans):
    lengths, needed, steps = plans
    n_steps = 0
    for pg in SIZES:
        lens = lengths[pg]
        for n in range(3 * pg + 6):
            plan = steps[pg, n]
            where = (pg, n, plan)
            assert sum(lens[i] for i, _, _, _ in plan) == n, where
            idx = [i for i, _, _, _ in plan]
            assert idx == sorted(idx), where                       # full-size steps first, then descending lengths
            short = [i for i in idx if i != 0]
            assert len(short) == len(set(short)), where            # each shorter length at most once
            before = 0
            for k, (i, pre, start, tail) in enumerate(plan):
                if k == 0:
                    assert (pre, start) == (0, 0), where           # head-sampled on set 0
                else:
                    assert (pre, start) == (1, before & 1), where  # pre-sampled where the replays before it left their draw
                assert tail == (1 if k + 1 < len(plan) else 0), where
                assert needed[pg, lens[i]][pre * 4 + start * 2 + tail] == 1, where
                before += lens[i]
            n_steps += len(plan)
    assert n_steps > 0
