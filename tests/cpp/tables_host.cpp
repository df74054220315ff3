// tests/cpp/tables_host.cpp -- builds the per-matrix tables on the host alone (ie_tables.cpp, no
// device, no library) and prints EncTables::c, the N x N cos products ie_cos_table reads back, as
// hex floats, one per line.  usage: tables_host MATRIX_FILE N
// tests/test_tables_host.py compiles it with the host sanitizers and compares the output with
// tests/golden/cos_table.json.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "ie_ctx.hpp"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    const int n = std::atoi(argv[2]);
    if (n != 4 && n != 8) return 2;
    std::vector<uint16_t> q;
    FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    for (unsigned v; std::fscanf(f, "%u", &v) == 1;) q.push_back(uint16_t(v));
    std::fclose(f);
    if (int(q.size()) != n * n) return 2;
    auto T = std::make_unique<ie::EncTables>();
    if (!iec::build_tables(n, q.data(), T.get())) {
        std::fprintf(stderr, "FP32 transform does not match the reference map\n");
        return 1;
    }
    for (int k = 0; k < n * n; k++) std::printf("%a\n", T->c[k]);
    return 0;
}
