// The template's edge graph for the sparse N-ICP step (nicp_sparse.hip): CSR adjacency, vertex degrees and connected components from
// the unique edges p1 < p2 < n of the C ABI.  Plain C++ for the host, no HIP: the library calls it once per handle and
// tests/c/nicp_graph_driver.cpp feeds it edge lists under the sanitizers.
//     row_ptr[n + 1], col[2E]   neighbours of vertex i = col[row_ptr[i] .. row_ptr[i + 1]), ASCENDING (whatever the order of the edges)
//     degree[n]                 row_ptr[i + 1] - row_ptr[i]
//     component[n]              labels 0 .. n_components - 1, numbered by each component's lowest vertex; an isolated vertex is its own
// A repeated edge is an error here (the dense path counts it twice in the degree and once off the diagonal: neither the reference's
// Set of edges nor a consistent matrix).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

enum { NICP_GRAPH_OK = 0, NICP_GRAPH_BAD_EDGE = 1, NICP_GRAPH_DUPLICATE_EDGE = 2, NICP_GRAPH_TOO_LARGE = 3 };

struct NicpGraph {
    int64_t n = 0;
    std::vector<int32_t> row_ptr, col, degree, component;
    int32_t n_components = 0;
};

// *bad_edge (nullable) = the index of the first offending edge
inline int nicp_graph_build(int64_t n, int64_t n_edges, const int32_t *edges, NicpGraph *g, int64_t *bad_edge) {
    if (bad_edge) *bad_edge = -1;
    if (n < 1 || n_edges < 0 || n > INT32_MAX || n_edges > INT32_MAX / 2) return NICP_GRAPH_TOO_LARGE;
    g->n = n;
    g->degree.assign((size_t)n, 0);
    for (int64_t e = 0; e < n_edges; ++e) {
        const int32_t p1 = edges[2 * e], p2 = edges[2 * e + 1];
        if (p1 < 0 || p2 <= p1 || p2 >= n) {
            if (bad_edge) *bad_edge = e;
            return NICP_GRAPH_BAD_EDGE;
        }
        ++g->degree[(size_t)p1];
        ++g->degree[(size_t)p2];
    }
    g->row_ptr.assign((size_t)n + 1, 0);
    for (int64_t i = 0; i < n; ++i) g->row_ptr[(size_t)i + 1] = g->row_ptr[(size_t)i] + g->degree[(size_t)i];
    g->col.assign((size_t)(2 * n_edges), 0);
    std::vector<int32_t> fill(g->row_ptr.begin(), g->row_ptr.end() - 1);
    for (int64_t e = 0; e < n_edges; ++e) {
        const int32_t p1 = edges[2 * e], p2 = edges[2 * e + 1];
        g->col[(size_t)fill[(size_t)p1]++] = p2;
        g->col[(size_t)fill[(size_t)p2]++] = p1;
    }
    for (int64_t i = 0; i < n; ++i) {
        int32_t *a = g->col.data() + g->row_ptr[(size_t)i], *b = g->col.data() + g->row_ptr[(size_t)i + 1];
        std::sort(a, b);
        const int32_t *dup = std::adjacent_find(a, b);
        if (dup != b) {
            if (bad_edge) {  // the second occurrence of the pair in the caller's list
                const int32_t lo = std::min<int32_t>((int32_t)i, *dup), hi = std::max<int32_t>((int32_t)i, *dup);
                int seen = 0;
                for (int64_t e = 0; e < n_edges; ++e)
                    if (edges[2 * e] == lo && edges[2 * e + 1] == hi && ++seen == 2) {
                        *bad_edge = e;
                        break;
                    }
            }
            return NICP_GRAPH_DUPLICATE_EDGE;
        }
    }
    // components: breadth first from every vertex not reached yet, in ascending order
    g->component.assign((size_t)n, -1);
    g->n_components = 0;
    std::vector<int32_t> queue;
    queue.reserve((size_t)n);
    for (int64_t s = 0; s < n; ++s) {
        if (g->component[(size_t)s] >= 0) continue;
        const int32_t label = g->n_components++;
        queue.clear();
        queue.push_back((int32_t)s);
        g->component[(size_t)s] = label;
        for (size_t head = 0; head < queue.size(); ++head) {
            const int32_t i = queue[head];
            for (int32_t k = g->row_ptr[(size_t)i]; k < g->row_ptr[(size_t)i + 1]; ++k) {
                const int32_t j = g->col[(size_t)k];
                if (g->component[(size_t)j] < 0) {
                    g->component[(size_t)j] = label;
                    queue.push_back(j);
                }
            }
        }
    }
    return NICP_GRAPH_OK;
}

// The normal equations alpha^2 Lg (x) G^2 + (block-diagonal data term) are singular exactly when a component of the graph holds no
// vertex with a data term (a non-zero weight or a landmark term): the Laplacian's constant vector of that component is in the null
// space.  has_term[n]: non-zero where vertex i has one.  Returns the lowest component without any, or -1.  `seen` is scratch the
// caller may keep across calls (resized here).
inline int32_t nicp_graph_unanchored_component(const NicpGraph &g, const uint8_t *has_term, std::vector<uint8_t> &seen) {
    seen.assign((size_t)g.n_components, 0);
    for (int64_t i = 0; i < g.n; ++i)
        if (has_term[i]) seen[(size_t)g.component[(size_t)i]] = 1;
    for (int32_t c = 0; c < g.n_components; ++c)
        if (!seen[(size_t)c]) return c;
    return -1;
}
