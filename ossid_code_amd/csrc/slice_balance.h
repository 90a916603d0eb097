// Slices of equal WORK for the persistent SA kernels (SPEC 4.5): wave w of nw walks the centres from the first one whose
// exclusive prefix cost is >= w * W / nw up to where wave w + 1 starts, W the total cost. The costs come from the ball query:
// one total per (hypothesis, ball-query workgroup) and each centre's hit count. Plain arithmetic, stated once for both
// kernels and for the host program that checks it (tests/slice_balance_check.cpp): no output of a kernel depends on where
// the slices are cut, but a boundary outside [0, total] would be an out-of-bounds gather.
//
// The search is cut so that 64 lanes can share it: a lane answers for one contiguous chunk of the totals (lane_part_sum)
// and of the straddled workgroup's centres (lane_centre_sum); the walk over those 64 sums, over one chunk's totals and over
// one chunk's centres is serial and the same in every lane. On the host the "lanes" are a loop.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SLICE_HD __host__ __device__ inline
#else
#define SLICE_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define SLICE_UNIFORM(x) __builtin_amdgcn_readfirstlane(x)      // the walk is wave-uniform: keep it in scalar registers
#else
#define SLICE_UNIFORM(x) (x)
#endif

constexpr int SLICE_LANES = 64;

struct SliceCosts {
    const int* part;             // cost total of each ball-query workgroup, hypothesis-major: [B][ppb]
    const unsigned char* cnt;    // hits of each centre, capped at 64: [B * np]
    int nparts, ppb, cpb;        // B * ppb; workgroups per hypothesis; centres per workgroup (the hypothesis's last: the rest)
    int np, total;               // centres per hypothesis, B * np
    int sa2;                     // the unit: 0 = SA1's granules of 8 columns, 1 = SA2's half tiles
};

// what the SA kernel spends on a centre with `cnt` hits
SLICE_HD int centre_cost(int cnt, int sa2) {
    if (sa2) return cnt <= 48 ? 3 : 4;
    const int d = cnt < 1 ? 1 : cnt > 64 ? 64 : cnt;
    return (d + 7) >> 3;
}

SLICE_HD int slice_min(int a, int b) { return a < b ? a : b; }
SLICE_HD int part_chunk(const SliceCosts& s) { return (s.nparts + SLICE_LANES - 1) / SLICE_LANES; }
SLICE_HD int centre_chunk(const SliceCosts& s) { return (s.cpb + SLICE_LANES - 1) / SLICE_LANES; }

SLICE_HD int lane_part_sum(const SliceCosts& s, int lane) {
    const int per = part_chunk(s), a = slice_min(lane * per, s.nparts), b = slice_min(a + per, s.nparts);
    int sum = 0;
    for (int i = a; i < b; ++i) sum += s.part[i];
    return sum;
}

// the centres [c0, c1) that workgroup p of the ball query answered for
SLICE_HD void part_centres(const SliceCosts& s, int p, int& c0, int& c1) {
    const int hyp = p / s.ppb, y = p % s.ppb;
    c0 = hyp * s.np + slice_min(y * s.cpb, s.np);
    c1 = slice_min(c0 + s.cpb, hyp * s.np + s.np);
}

SLICE_HD int lane_centre_sum(const SliceCosts& s, int p, int lane) {
    int c0, c1;
    part_centres(s, p, c0, c1);
    const int per = centre_chunk(s), a = slice_min(c0 + lane * per, c1), b = slice_min(a + per, c1);
    int sum = 0;
    for (int i = a; i < b; ++i) sum += centre_cost(s.cnt[i], s.sa2);
    return sum;
}

// Skips the leading elements that end before `target`: returns the first k whose inclusive prefix reaches it (n for none),
// `run` advanced over the skipped ones. Every centre of a skipped element has an exclusive prefix below the target.
template <class Get>
SLICE_HD int slice_skip(Get get, int n, long long target, long long& run) {
    int k = 0;
    while (k < n) {
        const int v = get(k);
        if (run + v >= target) break;
        run += v;
        ++k;
    }
    return k;
}

// The first centre whose exclusive prefix cost is >= target: in [0, total], not decreasing in target, 0 for target <= 0 and
// total for target >= W. lane_sums(k) is lane_part_sum of lane k; fill(p) makes the 64 lane_centre_sum values of workgroup
// p and returns their accessor.
template <class LaneSums, class Fill>
SLICE_HD int slice_boundary(const SliceCosts& s, long long target, LaneSums lane_sums, Fill fill) {
    if (target <= 0) return 0;
    long long run = 0;
    const int per = part_chunk(s);
    const int k1 = slice_skip(lane_sums, SLICE_LANES, target, run);
    const int p0 = k1 * per, n = slice_min(per, s.nparts - p0);
    if (k1 == SLICE_LANES || n <= 0) return s.total;
    const int kp = slice_skip([&](int i) { return SLICE_UNIFORM(s.part[p0 + i]); }, n, target, run);
    if (kp == n) return s.total;
    const int p = p0 + kp;
    auto centre_sums = fill(p);
    const int k2 = slice_skip(centre_sums, SLICE_LANES, target, run);
    int c0, c1;
    part_centres(s, p, c0, c1);
    int i = slice_min(c0 + slice_min(k2, SLICE_LANES) * centre_chunk(s), c1);
    while (i < c1 && run < target) run += centre_cost(SLICE_UNIFORM((int)s.cnt[i]), s.sa2), ++i;
    return i < 0 ? 0 : i > s.total ? s.total : i;
}

// [first, end) of wave w of nw. The last wave ends at total whatever the costs say, and end is never below first.
template <class LaneSums, class Fill>
SLICE_HD void slice_bounds(const SliceCosts& s, int w, int nw, LaneSums lane_sums, Fill fill, int& first, int& end) {
    long long W = 0;
    for (int k = 0; k < SLICE_LANES; ++k) W += lane_sums(k);
    first = slice_boundary(s, (long long)w * W / nw, lane_sums, fill);
    end = w + 1 >= nw ? s.total : slice_boundary(s, (long long)(w + 1) * W / nw, lane_sums, fill);
    if (end < first) end = first;
}
