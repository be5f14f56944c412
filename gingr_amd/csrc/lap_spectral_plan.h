// Every decision of the sparse inverse-Laplacian model build (lap_spectral.hip; C ABI: gingr_model_from_laplacian) -- the edge list of
// a triangulation, the width of the iteration block, the Chebyshev filter's interval, degree and recurrence coefficients, the stop
// rule.  Plain C++ for the host, no HIP: the library calls it, tests/c/lap_spectral_plan_driver.cpp runs it under the sanitizers and
// tests/lap_spectral_restatement.py restates it in numpy.
//
// The iteration (Chebyshev-filtered subspace iteration for the SMALLEST eigenpairs of L = D - A, no inner solves):
//     X [n][m]          the block, deflated against the constant vector of every connected component (the null space of L)
//     one outer step    Y = p_d(L) X with p_d the degree-d Chebyshev polynomial of the interval [a, Lambda] scaled to p_d(0) = 1;
//                       deflate; Cholesky-QR twice; Rayleigh-Ritz; residuals |L x - theta x| / Lambda of the wanted pairs
//     Lambda            2 max degree: the Gershgorin bound of the spectrum
//     a                 the largest Ritz value of the block as it stands: what lies above it is damped, what lies below amplified
// p_d is at most 1 in magnitude on [a, Lambda] and grows monotonically towards 0, where it is exactly 1 by the scaling, so after a
// filter step no direction of the block is larger than 1 and the least amplified of its own directions (the Ritz vector of a) is
// 1 / T_d(c / e) of that, c = (Lambda + a) / 2, e = (Lambda - a) / 2.  The degree of a step is the largest d that keeps this spread
// below kLapSpreadBound -- whatever the Ritz values below a are, so an inaccurate early block cannot mislead the rule -- and the Gram
// matrix of the filtered block then has a condition number below the bound squared: the first Cholesky factorisation cannot break
// down in float64, the second sees a block that is orthonormal to rounding.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

constexpr int kLapMaxPairs = 170;             // 3 k <= 512, a model's rank limit
constexpr int kLapMaxBlock = 192;             // the Ritz problem stays on the register eigen-kernel (kSymEigColsMaxN)
constexpr int kLapMinGuard = 8;               // columns beyond the wanted ones: they set the convergence rate of the last wanted pair
constexpr double kLapCutoff = 1e-5;           // eigenvalues up to this are dropped (MatrixHelper.pinv, MatrixHelper.scala:21-26)
constexpr double kLapDefaultTolerance = 1e-10;
constexpr double kLapSpreadBound = 1e6;       // largest ratio between two directions of a filtered block
constexpr int kLapMaxStepDegree = 512;
// Default budget of block products with L: four times the largest total observed on one MI355X, rounded up -- femur (1 622 vertices)
// 166 at k = 34 and 165 at k = 170, a closed hull of 50 000 vertices 956 and 785 (profiles/laplacian_model_50000.json).  The margin is
// for meshes more elongated than those (a smaller mu_k / Lambda needs more degree: a flat band of 2 x 1 200 vertices, whose
// smallest non-zero eigenvalue is already below the cut-off, takes 937 at k = 3).
constexpr int kLapDefaultMaxDegree = 4000;

enum { LAP_EDGES_OK = 0, LAP_EDGES_BAD_INDEX = 1, LAP_EDGES_TOO_LARGE = 2, LAP_EDGES_NO_CELLS = 3 };

// The unique undirected edges p1 < p2 of a triangulation, ascending by (p1, p2): what nicp_graph_build takes.  A cell that names a
// vertex twice contributes no loop (LaplacianHelper clears the diagonal of its adjacency); a repeated triangle or a shared edge counts
// once.  *bad_cell (nullable): the first cell with an index outside [0, n).
inline int lap_edges_from_cells(int64_t n, int64_t n_cells, const int32_t *cells, std::vector<int32_t> *edges, int64_t *bad_cell) {
    if (bad_cell) *bad_cell = -1;
    edges->clear();
    if (n_cells < 1) return LAP_EDGES_NO_CELLS;
    if (n < 1 || n > INT32_MAX || n_cells > INT32_MAX / 6) return LAP_EDGES_TOO_LARGE;
    std::vector<uint64_t> keys;
    keys.reserve((size_t)(3 * n_cells));
    for (int64_t c = 0; c < n_cells; ++c) {
        const int32_t *t = cells + 3 * c;
        for (int q = 0; q < 3; ++q)
            if (t[q] < 0 || t[q] >= n) {
                if (bad_cell) *bad_cell = c;
                return LAP_EDGES_BAD_INDEX;
            }
        for (int q = 0; q < 3; ++q) {
            const int32_t a = t[q], b = t[(q + 1) % 3];
            if (a == b) continue;
            keys.push_back(((uint64_t)(uint32_t)std::min(a, b) << 32) | (uint32_t)std::max(a, b));
        }
    }
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    edges->reserve(2 * keys.size());
    for (const uint64_t key : keys) {
        edges->push_back((int32_t)(key >> 32));
        edges->push_back((int32_t)(key & 0xffffffffu));
    }
    return LAP_EDGES_OK;
}

// The block: m columns in memory (a multiple of 16, at most kLapMaxBlock), of which the leading `active` are iterated -- all of them
// unless the deflated space has fewer dimensions (a tetrahedron: 3), where the Rayleigh-Ritz step is exact and no filter runs.
struct LapBlock {
    int m = 0, active = 0;
};
// k wanted pairs, dim = n - (number of connected components) >= k
inline LapBlock lap_block_plan(int k, int64_t dim) {
    LapBlock b;
    b.m = std::min(kLapMaxBlock, (k + kLapMinGuard + 15) / 16 * 16);
    b.active = (int)std::min<int64_t>(b.m, dim);
    return b;
}

// One filter step: the interval [a, bound], its centre c and half-width e, the degree and sigma_1 of the scaled recurrence
struct LapFilter {
    double a = 0, bound = 0, c = 0, e = 0, sigma1 = 0;
    int degree = 0;
};
// theta_max: the largest Ritz value of the block; bound: Lambda; max_degree: what the budget still allows (>= 1)
inline LapFilter lap_filter_plan(double theta_max, double bound, int max_degree) {
    LapFilter f;
    f.bound = bound;
    // (a Ritz value never exceeds Lambda; one within 5 % of it only arises from a start block on a graph of a few vertices more than the
    // block is wide, and a lower edge inside the block merely damps the block's top directions)
    f.a = std::min(std::max(theta_max, 1e-12 * bound), 0.95 * bound);
    f.c = 0.5 * (bound + f.a);
    f.e = 0.5 * (bound - f.a);
    f.sigma1 = -f.e / f.c;  // e / (0 - c): the polynomial is scaled at 0, the lower end of the spectrum
    const double d = std::floor(std::acosh(kLapSpreadBound) / std::acosh(f.c / f.e));
    f.degree = (int)std::min<double>(std::max(d, 1.0), (double)std::min(max_degree, kLapMaxStepDegree));
    return f;
}
// T_d(c / e): the spread the degree rule bounds
inline double lap_filter_spread(const LapFilter &f, int degree) { return std::cosh(degree * std::acosh(f.c / f.e)); }

// T_next = alpha (L T_cur) + beta T_cur + gamma T_prev, step = 1 .. degree (step 1: gamma = 0, T_cur = X).  *sigma carries the
// recurrence's state from step to step (the scaled three-term recurrence of Zhou and Saad: magnitudes stay bounded by 1).
struct LapStep {
    double alpha, beta, gamma;
};
inline LapStep lap_recurrence_step(const LapFilter &f, int step, double *sigma) {
    if (step <= 1) {
        *sigma = f.sigma1;
        return LapStep{f.sigma1 / f.e, -f.sigma1 * f.c / f.e, 0.0};
    }
    const double next = 1.0 / (2.0 / f.sigma1 - *sigma);
    const LapStep s{2.0 * next / f.e, -2.0 * next * f.c / f.e, -(*sigma) * next};
    *sigma = next;
    return s;
}

// The stop rule: every wanted pair's |L x - theta x| / Lambda is a number at or below the tolerance
inline bool lap_converged(const double *relative_residual, int wanted, double tolerance) {
    for (int j = 0; j < wanted; ++j)
        if (!(relative_residual[j] <= tolerance)) return false;
    return true;
}
// Ritz values (ascending) of the wanted pairs at or below the cut-off: they are dropped, so that many more pairs are wanted
inline int lap_count_dropped(const double *theta, int wanted) {
    int t = 0;
    while (t < wanted && theta[t] <= kLapCutoff) ++t;
    return t;
}
