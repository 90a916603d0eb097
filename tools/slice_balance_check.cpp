// Host check of csrc/slice_balance.h, the arithmetic that cuts the persistent SA kernels' work-balanced slices. A wrong
// boundary there is an out-of-bounds gather on the GPU, so this runs on the CPU first, built with
// -fsanitize=address,undefined (tests/test_slice_balance.py does that). For random and adversarial hit counts it shows that
//   the slices of waves 0 .. nw-1 tile [0, total) exactly and in order,
//   each boundary is the first centre whose exclusive prefix cost is >= w * W / nw (a brute-force scan says so),
//   no slice costs more than W / nw plus one centre's cost plus the rounding of the two targets.
// The 64 lanes of the device are a loop here; every other line is the header's.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../ossid_code_amd/csrc/slice_balance.h"

static int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (++failures < 20) {                        \
                std::fprintf(stderr, "FAIL %s: ", #cond);          \
                std::fprintf(stderr, __VA_ARGS__);       \
                std::fprintf(stderr, "\n");              \
            }                                             \
        }                                                 \
    } while (0)

struct Case {
    const char* name;
    int B, np, cpb, nw, sa2;
    std::vector<unsigned char> cnt;
};

static void run(const Case& c, bool verbose) {
    const int total = c.B * c.np, ppb = (c.np + c.cpb - 1) / c.cpb, nparts = c.B * ppb;
    // exactly-sized heap arrays: a read past either end is an AddressSanitizer report
    std::vector<int> part(nparts);
    std::vector<long long> excl(total + 1, 0);
    int cmax = 0;
    for (int i = 0; i < total; ++i) {
        const int k = centre_cost(c.cnt[i], c.sa2);
        excl[i + 1] = excl[i] + k;
        cmax = k > cmax ? k : cmax;
        part[(i / c.np) * ppb + (i % c.np) / c.cpb] += k;
    }
    const long long W = excl[total];
    SliceCosts s{part.data(), c.cnt.data(), nparts, ppb, c.cpb, c.np, total, c.sa2};
    int la[SLICE_LANES], lc[SLICE_LANES];
    for (int k = 0; k < SLICE_LANES; ++k) la[k] = lane_part_sum(s, k);
    auto lane_sums = [&](int k) { return la[k]; };
    auto fill = [&](int p) {
        for (int k = 0; k < SLICE_LANES; ++k) lc[k] = lane_centre_sum(s, p, k);
        return [&](int k) { return lc[k]; };
    };
    int prev_end = 0, empty = 0;
    long long worst = 0;
    for (int w = 0; w < c.nw; ++w) {
        int first = -1, end = -1;
        slice_bounds(s, w, c.nw, lane_sums, fill, first, end);
        CHECK(first == prev_end, "%s wave %d: first %d, previous end %d", c.name, w, first, prev_end);
        CHECK(first >= 0 && first <= end && end <= total, "%s wave %d: [%d, %d) of %d", c.name, w, first, end, total);
        if (first < 0 || end > total || first > end) return;
        const long long t0 = (long long)w * W / c.nw, t1 = (long long)(w + 1) * W / c.nw;
        int brute = 0;
        while (brute < total && excl[brute] < t0) ++brute;
        CHECK(first == brute, "%s wave %d: first %d, scan says %d", c.name, w, first, brute);
        const long long cost = excl[end] - excl[first];
        // excl[first] is in [t0, t0 + cmax) and excl[end] in [t1, t1 + cmax); t1 - t0 <= W / nw + 1
        CHECK(cost <= W / c.nw + 1 + cmax, "%s wave %d: cost %lld of W %lld / %d, cmax %d", c.name, w, cost, W, c.nw, cmax);
        worst = cost > worst ? cost : worst;
        empty += first == end;
        prev_end = end;
    }
    CHECK(prev_end == total, "%s: the last slice ends at %d of %d", c.name, prev_end, total);
    if (verbose)
        std::printf("%-28s total %7d W %8lld nw %5d  worst slice %6lld (W/nw %.1f)  empty %d\n", c.name, total, W, c.nw, worst,
                (double)W / c.nw, empty);
}

int main() {
    std::mt19937 rng(12345);
    auto fill = [&](int n, int lo, int hi) {
        std::vector<unsigned char> v(n);
        std::uniform_int_distribution<int> d(lo, hi);
        for (auto& x : v) x = (unsigned char)d(rng);
        return v;
    };
    std::vector<Case> cases;
    for (int sa2 = 0; sa2 < 2; ++sa2) {
        cases.push_back({"all equal (full rows)", 1000, sa2 ? 128 : 512, 256, 1024, sa2, fill(1000 * (sa2 ? 128 : 512), 64, 64)});
        cases.push_back({"bench shape, random", 1000, sa2 ? 128 : 512, 256, 1024, sa2, fill(1000 * (sa2 ? 128 : 512), 30, 64)});
        cases.push_back({"one hypothesis", 1, 512, 256, 1024, sa2, fill(512, 0, 64)});
        cases.push_back({"one hypothesis, 16 waves", 1, 512, 256, 16, sa2, fill(512, 0, 64)});
        cases.push_back({"total < nw", 3, 32, 256, 1024, sa2, fill(96, 0, 64)});
        cases.push_back({"costs of 1 only", 9, 512, 256, 16, sa2, fill(9 * 512, 0, 8)});
        cases.push_back({"costs of 1 only, many waves", 9, 512, 256, 1024, sa2, fill(9 * 512, 1, 1)});
        cases.push_back({"odd totals", 7, 96, 256, 13, sa2, fill(7 * 96, 0, 64)});
        cases.push_back({"odd totals, LDS-form parts", 11, 1056, 512, 37, sa2, fill(11 * 1056, 0, 64)});
        cases.push_back({"np not a multiple of cpb", 5, 800, 256, 1021, sa2, fill(5 * 800, 0, 64)});
        cases.push_back({"one wave", 9, 128, 256, 1, sa2, fill(9 * 128, 0, 64)});
        cases.push_back({"more parts than lanes * 32", 4100, 32, 256, 1024, sa2, fill(4100 * 32, 0, 64)});
        // adversarial: all the cost at one end, and alternating extremes
        auto head = fill(9 * 512, 1, 1);
        for (int i = 0; i < 300; ++i) head[i] = 64;
        cases.push_back({"heavy head", 9, 512, 256, 64, sa2, head});
        auto tail = fill(9 * 512, 1, 1);
        for (int i = 0; i < 300; ++i) tail[tail.size() - 1 - i] = 64;
        cases.push_back({"heavy tail", 9, 512, 256, 64, sa2, tail});
        auto alt = fill(9 * 512, 1, 1);
        for (size_t i = 0; i < alt.size(); i += 2) alt[i] = 64;
        cases.push_back({"alternating 1 / 64", 9, 512, 256, 1024, sa2, alt});
    }
    for (int trial = 0; trial < 300; ++trial) {
        const int B = 1 + rng() % 40, np = 32 * (1 + rng() % 20), cpb = rng() % 2 ? 256 : 512, nw = 1 + rng() % 1500;
        const int lo = rng() % 65, hi = lo + rng() % (65 - lo);
        cases.push_back({"random", B, np, cpb, nw, (int)(rng() % 2), fill(B * np, lo, hi)});
    }
    for (size_t i = 0; i < cases.size(); ++i) {
        run(cases[i], i < 30);     // the named ones print a line each
    }
    std::fprintf(stderr, failures ? "slice_balance_check: %d FAILURES\n" : "slice_balance_check: ok (%d cases)\n",
                 failures ? failures : (int)cases.size());
    return failures ? 1 : 0;
}
