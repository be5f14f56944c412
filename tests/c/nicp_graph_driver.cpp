// Host driver of the N-ICP edge graph (gingr_amd/csrc/nicp_graph.h) for tests/test_nicp_graph_host.py.  Raw int32 on stdin until it
// ends, raw int32 on stdout.  One record in: {n, E, edges[2E], has_term[n]}; out: {status, bad_edge, n_components, unanchored} and, for
// status 0, row_ptr[n + 1], col[2E], degree[n], component[n].  Plain C++ for the host compiler: the header carries no device code.
#include <cstdio>
#include <vector>

#include "nicp_graph.h"

static bool get(int32_t *p, size_t n) { return n == 0 || fread(p, sizeof(int32_t), n, stdin) == n; }
static bool put(const std::vector<int32_t> &v) { return v.empty() || fwrite(v.data(), sizeof(int32_t), v.size(), stdout) == v.size(); }

int main() {
    int32_t head[2];
    std::vector<uint8_t> seen;
    while (fread(head, sizeof(int32_t), 2, stdin) == 2) {
        if (head[0] < 1 || head[1] < 0) return 2;
        const size_t n = (size_t)head[0], E = (size_t)head[1];
        std::vector<int32_t> edges(2 * E), term(n);
        if (!get(edges.data(), edges.size()) || !get(term.data(), n)) return 1;
        std::vector<uint8_t> has(term.begin(), term.end());
        NicpGraph g;
        int64_t bad = -1;
        const int status = nicp_graph_build((int64_t)n, (int64_t)E, edges.data(), &g, &bad);
        std::vector<int32_t> out{status, (int32_t)bad, 0, -1};
        if (status == NICP_GRAPH_OK) {
            out[2] = g.n_components;
            out[3] = nicp_graph_unanchored_component(g, has.data(), seen);
        }
        if (!put(out)) return 1;
        if (status == NICP_GRAPH_OK && !(put(g.row_ptr) && put(g.col) && put(g.degree) && put(g.component))) return 1;
    }
    return 0;
}
