// host_ffm_harness.cpp — the field-aware FM's host dataset build (fmhip_host.cpp: ffm_validate, ffm_build) as a stand-alone program under
// -fsanitize=address,undefined:  host_ffm_harness layout <file> <batch_rows> <chunk>, <file> one row per line, "field:feature:value ...".
// Prints ffm_validate's verdict and, for valid data, the layout in the words of tests/ffm_ref.py's layout(); every chunk's occurrences
// are read through the chunk tables (chunk_col, chunk0, cptr), the way k_ffm_backward finds them.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../sparkfm_amd/csrc/fmhip_host.h"

using namespace fmhip::host;

int main(int argc, char **argv) {
    if (argc != 5 || strcmp(argv[1], "layout") != 0) return 2;
    FILE *fh = fopen(argv[2], "r");
    if (!fh) return 2;
    std::vector<int64_t> row_ptr{0};
    std::vector<int32_t> col, field;
    std::vector<double> val;
    char line[1 << 16];
    while (fgets(line, sizeof line, fh)) {
        for (char *tok = strtok(line, " \n"); tok; tok = strtok(nullptr, " \n")) {
            int f, i;
            double v;
            if (sscanf(tok, "%d:%d:%lf", &f, &i, &v) != 3) return 2;
            field.push_back(f);
            col.push_back(i);
            val.push_back(v);
        }
        row_ptr.push_back((int64_t)col.size());
    }
    fclose(fh);
    const int64_t n_rows = (int64_t)row_ptr.size() - 1, batch_rows = atoll(argv[3]);
    const int chunk = atoi(argv[4]);
    const FfmCheck c = ffm_validate(n_rows, row_ptr.data(), col.data(), field.data(), val.data());
    printf("check %d %lld %lld %d %d %d\n", c.kind, (long long)c.row, (long long)c.entry, c.dim, c.fields, c.max_len);
    if (c.kind != kFfmOk) return 0;
    FfmLayout L;
    ffm_build(n_rows, row_ptr.data(), col.data(), field.data(), val.data(), batch_rows, chunk, &L);
    for (int64_t r = 0; r < n_rows; ++r) {
        printf("row %lld:", (long long)r);
        for (int64_t p = row_ptr[r]; p < row_ptr[r + 1]; ++p) printf(" %d:%d:%d", L.field[(size_t)p], L.col[(size_t)p], L.run[(size_t)p]);
        printf("%s\n", row_ptr[r] == row_ptr[r + 1] ? " " : "");
    }
    for (size_t b = 0; b < L.batches.size(); ++b) {
        const FfmBatch &B = L.batches[b];
        const int32_t *cptr = L.cptr.data() + B.cptr_off, *chunk0 = L.chunk0.data() + B.cptr_off, *ccol = L.chunk_col.data() + B.chunk_off;
        std::vector<std::string> occ((size_t)B.n_cols);
        for (int32_t ch = 0; ch < B.n_chunks; ++ch) {
            const int32_t cc = ccol[ch];
            if (cc < 0 || cc >= B.n_cols || ch < chunk0[cc] || ch >= chunk0[cc + 1]) return 1;
            const int32_t lo = cptr[cc] + chunk * (ch - chunk0[cc]), hi = std::min(lo + chunk, cptr[cc + 1]);
            for (int32_t o = lo; o < hi; ++o) {
                char buf[32];
                snprintf(buf, sizeof buf, " %d.%d", L.occ_row[(size_t)(B.nnz0 + o)], L.occ_pos[(size_t)(B.nnz0 + o)]);
                occ[(size_t)cc] += buf;
            }
        }
        for (int32_t cc = 0; cc < B.n_cols; ++cc)
            printf("batch %zu col %d chunks %d:%s\n", b, L.cfeat[(size_t)(B.col_off + cc)], chunk0[cc + 1] - chunk0[cc], occ[(size_t)cc].c_str());
    }
    return 0;
}
