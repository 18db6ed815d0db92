// fmhip_ffm_dataset.h — the FFM dataset handle (include/fmhip_ffm.h), shared by the units whose models train on it: fmhip_ffm.hip
// builds and owns it, fmhip_fwfm.hip reads it.
#pragma once
#include "fmhip_internal.h"

#include <vector>

struct fmhip_ffm_dataset {
    template <typename T> using DevBuf = fmhip::host::DevBuf<T>;
    int device = 0;
    int64_t n_rows = 0, nnz = 0, batch_rows = 0, max_rows = 0;
    int32_t dim = 0, fields = 0, max_len = 0, max_chunks = 0;
    bool labels = false;
    std::vector<fmhip::host::FfmBatch> batches;
    DevBuf<int64_t> row_ptr;
    DevBuf<int32_t> col, cfeat, cptr, chunk0, chunk_col, occ_row;
    DevBuf<uint8_t> fld, run, occ_pos;
    DevBuf<float> val, y;
};
