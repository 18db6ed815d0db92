// fmhip_mcmc_handle.h — the MCMC learner's handle (internal to libfmhip.so): fmhip_mcmc.hip makes it over a flat dataset and runs its
// epoch; fmhip_mcmc_relational.hip makes it over a relational dataset (include/fmhip_mcmc_relational.h), and fmhip_mcmc_epoch hands
// such a handle's epoch to mcmc_relational_epoch.  Every other call of fmhip_mcmc.h works on either kind.
#pragma once
#include "fmhip_internal.h"
#include "als_kernels.h"
#include "../../include/fmhip_mcmc_groups.h"

#include <memory>
#include <vector>

// What a relational handle holds beside the state: the parts (the relations in the order given, then the plain part), the order
// they are walked in, and the fp64 workspace of the block-structure sweep (mcmc_blocks.h).
struct McmcRelational {
    template <typename T> using DevBuf = fmhip::host::DevBuf<T>;
    struct Part {
        fmhip_dataset_t d = nullptr;
        int32_t rel = -1;                   // index into the relational dataset's relations; -1: the plain part
        std::vector<int32_t> h_trained;     // [n_cols] 1: the column is in T
        int64_t n_trained = 0;
        DevBuf<int32_t> trained;
        DevBuf<double> n, cache, part;      // [J] n_p; the caches [kBlockCaches][J]; the long lists' chunk sums
        DevBuf<double> yhat, q, z, sums;    // yhat_p [J], q_p [k][J], the part's noise, k_block_theta_sums' partials
        std::vector<double> h_sums;
    };
    struct TestPart {
        DevBuf<double> yhat, q;
    };
    fmhip_relational_t train = nullptr, test = nullptr;
    std::vector<std::unique_ptr<Part>> parts;
    std::vector<int> order;                 // the parts by ascending id range: the walk's order
    bool part_groups = false;               // a part is an attribute group: lambda and mu are (k + 1) x parts
    DevBuf<double> e, Q, qrest, zeros, zbias, hyp;      // [N], [k][N], [N], max(J_p, N) zeros, the bias's noise, per part {alpha, lambda[k + 1], mu[k + 1]}
    std::vector<double> h_hyp;
    std::vector<std::unique_ptr<TestPart>> test_parts;
    DevBuf<double> test_zeros;
};

struct fmhip_mcmc {
    template <typename T> using DevBuf = fmhip::host::DevBuf<T>;
    fmhip_model_t m = nullptr;
    fmhip_dataset_t train = nullptr, test = nullptr;
    fmhip_mcmc_opts opts{};
    int32_t task = FMHIP_MCMC_REGRESSION;
    fmhip::McmcLink link;                   // what a draw's test prediction becomes before it joins the sum
    fmhip::host::McmcPriors priors;
    int32_t k = 0;
    int64_t n_trained = 0;                  // |T|: the column slots with id < num_attribute
    double alpha = 1.0;
    std::vector<double> lambda, mu;         // [(k + 1) * G], row-major: [g * G + a]
    int32_t G = 1;                          // attribute groups (include/fmhip_mcmc_groups.h); 1: none, the epoch fmhip_mcmc.h describes
    fmhip::host::McmcGroupPlan plan;        // G > 1: the chunks of the grouped sums
    int64_t plan_cols = 0;                  // ... and the column slots they were made over
    DevBuf<int32_t> d_group, d_order, d_chunk_ptr, d_chunk_group;      // group: [num_attribute + 1]
    DevBuf<double> gsums;                   // k_mcmc_group_sums' partials [n_chunks * (k + 1) * 2]
    std::vector<double> h_gsums;
    int64_t iterations = 0, draws = 0;
    DevBuf<double> z, hyp, sums;            // the epoch's noise; {alpha, lambda, mu}; k_mcmc_sums' partials
    DevBuf<double> ystar;                   // classification: the latent targets the last epoch trained on [train rows]
    DevBuf<double> test_sum, test_last, test_zero;     // [test rows]: the running sum, the last draw's predictions, zeros
    std::vector<double> h_sums, h_hyp;
    std::unique_ptr<McmcRelational> rel;    // a handle over relational data (include/fmhip_mcmc_relational.h): train is NULL, test a flat test set or NULL
};

namespace fmhip {
namespace host {
// fmhip_mcmc_epoch of a relational handle (the caller holds no lock)
int mcmc_relational_epoch(fmhip_mcmc_t s, fmhip_mcmc_stats *stats);
// ---- what the two creators and the two epochs share (fmhip_mcmc.hip) ----
// the settings a handle is made with: the defaults where opts / task_opts is NULL, refused when one is out of range
int mcmc_settings(const fmhip_mcmc_opts *opts, const fmhip_mcmc_task_opts *task_opts, fmhip_mcmc_opts *o, fmhip_mcmc_task_opts *to);
// every reason a flat test set is refused
int mcmc_check_test(fmhip_model_t m, fmhip_dataset_t test);
// the fields every handle has: the model, the settings, the priors, the task with its link, k
void mcmc_fill(fmhip_mcmc_t s, fmhip_model_t m, const fmhip_mcmc_opts &o, const fmhip_mcmc_task_opts &to);
// test_sum, test_last, test_zero: max(n_rows, 1) zeros each
int mcmc_alloc_test(fmhip_mcmc_t s, int64_t n_rows);
// the flat test set's rows under the draw the epoch left: into test_last, through the link, onto test_sum
int mcmc_accumulate_flat_test(fmhip_mcmc_t s);
// the epoch's end: the parameters back into the model, the counters, the stats (nullable)
int mcmc_finish_epoch(fmhip_mcmc_t s, double train_rmse, fmhip_mcmc_stats *stats);
}  // namespace host
}  // namespace fmhip
