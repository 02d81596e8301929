// posterior_ws.h -- shape limits, tiling and workspace layout of the posterior statistics (include/natinf_posterior.h), shared by the two
// translation units that touch the workspace: ni_step.hip (k_post_samples writes the planes) and posterior.hip (everything else).  Host code only.
#pragma once
#include <stdint.h>
#include "natinf_posterior.h"

namespace post {

constexpr int BM = 64;            // rows of s (i) per block of k_post_dots
constexpr int BN = 128;           // rows of f (j) per block
constexpr int BK = 64;            // values of k per LDS tile
constexpr int FLUSH_TILES = 8;    // the fp32 accumulators are added into the fp64 ones after 8 tiles = 512 values of k
constexpr int MAX_SPLITS = 32;
constexpr int RESIDENT_BLOCKS = 512;     // 256 CUs x 2 blocks (46 KB of LDS, <= 256 VGPRs each)

inline bool shape_ok(int n, int d) {
    return n >= 1 && n <= NATINF_POSTERIOR_MAX_N && d >= 64 && d <= NATINF_POSTERIOR_MAX_D && d % 64 == 0;
}

// Blocks over K: as many as make one round of resident blocks, rounded to nearest.  A function of (n, d) only, so the summation order -- and
// every bit of the result -- does not depend on the device.
inline int splits_for(int n, int d) {
    const int64_t tiles = (int64_t)((n + BM - 1) / BM) * ((n + BN - 1) / BN);
    const int ktiles = d / BK, smax = ktiles < MAX_SPLITS ? ktiles : MAX_SPLITS;
    const int64_t s = (2 * RESIDENT_BLOCKS + tiles) / (2 * tiles);
    return (int)(s < 1 ? 1 : (s > smax ? smax : s));
}

// doubles reserved for the partial sums: a bound of splits_for(n, d) * n^2 that is monotone in n and in d (the split count itself is not).
// round(x) <= 1.5 x for x >= 1 and n^2 <= tiles * BM * BN give splits * n^2 <= 1.5 * RESIDENT_BLOCKS * BM * BN whenever splits > 1.
inline int64_t partial_doubles(int n, int d) {
    const int64_t nn = (int64_t)n * n, round_cap = (int64_t)3 * RESIDENT_BLOCKS * BM * BN / 2;
    const int64_t by_blocks = nn > round_cap ? nn : round_cap, by_k = nn * (d / BK < MAX_SPLITS ? d / BK : MAX_SPLITS);
    return by_blocks < by_k ? by_blocks : by_k;
}

struct Layout {
    int splits;
    int64_t planes, norms, partials, total;       // byte offsets: bf16 [3][n][d], double [n], double [splits][n][n]
};

inline int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }

inline Layout layout(int n, int d) {
    Layout L;
    L.splits = splits_for(n, d);
    L.planes = 0;
    L.norms = align256(3 * (int64_t)n * d * 2);
    L.partials = L.norms + align256((int64_t)n * 8);
    L.total = L.partials + align256(partial_doubles(n, d) * 8);
    return L;
}

}  // namespace post
