// als_kernels.h — launchers of the fp64 ALS epoch and of the MCMC learner's epoch, which walks the same columns (internal to
// libfmhip.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fmhip {

struct AlsArgs {
    int32_t k;
    int64_t num_attribute;   // loop bound of the sweeps (arrays have num_attribute + 1 slots)
    int64_t n_rows;
    int64_t nnz;
    // rows (CSR, stored order) — fp64 values
    const int64_t *row_ptr;
    const int32_t *col;
    const double *val;
    const double *y;
    // the same rows with every row's entries sorted by feature id (stable): the per-row order in which the
    // reference's transposed q pass (S/fm/lib/ALS.scala:146-150) adds a row's terms
    const int32_t *scol;
    const double *sval;
    // transpose (compressed columns of the single batch) — fp64 values
    int32_t n_cols;
    const int32_t *cfeat;
    const int32_t *cptr;
    const uint32_t *crow;
    const double *cval;
    // fp64 parameters, reference layout v[f + i*k]
    double *w0, *w, *v;
    double reg0, regw, regv;
    // workspace: e[n_rows]; q[n_rows * k] (every factor's q comes from an up-front pass over the feature-sorted rows);
    // part[2 * kAlsMaxParts + 2]: per-workgroup partial sums of a long column's chip-wide step
    double *e, *q, *part;
    // level schedule (optional): the compressed columns sorted by (level, id) — columns of one level share no row and
    // their steps commute exactly (fmhip_dataset::als_lev_cols)
    const int32_t *lev_cols;
};

// What the MCMC epoch's walks take beside AlsArgs (include/fmhip_mcmc.h; the ALS epoch's kernels take AlsArgs alone, as ever):
// hyp = {alpha, lambda[k + 1], mu[k + 1]} of the groups g = 0 (w), 1 + f (factor f); z = this epoch's N(0,1) per (group, column
// slot), [(k + 1) * n_cols], then the bias's; sample = 0: every step takes the conditional's mean and z does not enter it;
// zi: set by the launcher of a long column's chip-wide step — that column's entry of z
struct McmcDev {
    const double *hyp;
    const double *z;
    int32_t sample;
    int64_t zi;
};

// ... and what a handle with attribute groups (include/fmhip_mcmc_groups.h, G = n_groups > 1) takes in McmcDev's place — a type of
// its own, so that the instantiations the ALS epoch and an ungrouped handle run keep their arguments and their code; z, sample and
// zi are McmcDev's, so what does not depend on the groups (the noise, the bias step) takes it as one:
// hyp = {alpha, lambda[(k + 1) * G], mu[(k + 1) * G]}, [g * G + a]; group[i] = feature i's attribute group, num_attribute + 1
// entries (the walks read a column's id a step ahead of the test that skips quirk Q1's slot)
struct McmcGroupDev : McmcDev {
    const int32_t *group;
    int32_t n_groups;
};

// The plan of the grouped hyper-parameter sums on the device (fmhip_host.h: McmcGroupPlan)
struct McmcGroupSums {
    const int32_t *order, *chunk_ptr, *chunk_group;
    int32_t n_chunks;
    double *out;             // [n_chunks * (k + 1) * 2]: chunk c's {sum theta, sum (theta - mu_ga)^2} of parameter group g at 2 * (c * (k + 1) + g)
};

// The probit link of a classification handle (include/fmhip_mcmc_task.h): k_mcmc_probit_targets stands where the epoch's first
// residual pass stood and fills ystar — which AlsArgs.y points at for the whole epoch — from the labels' signs
enum { kProbitStart = 0, kProbitSample = 1, kProbitMean = 2 };
struct McmcProbit {
    const double *labels;    // the dataset's own: the class is [y > 0]
    double *ystar;           // [n_rows]
    int32_t mode;            // kProbitStart: y* = +-1 (the handle's first epoch); kProbitSample: the truncated-normal draw; kProbitMean: its mean
};

// What a draw's test prediction becomes before it joins the running sum: itself, Phi of it, or itself clamped to [lo, hi]
enum { kLinkNone = 0, kLinkProbit = 1, kLinkClamp = 2 };
struct McmcLink {
    int32_t kind = kLinkNone;
    double lo = 0.0, hi = 0.0;
};

constexpr int kAlsMaxParts = 512;       // workgroups of a chip-wide column step
// Columns of at least this many entries take the chip-wide two-launch step, shorter ones the one-workgroup walk
// (FMHIP_ALS_LONG in the environment overrides it: a test / measurement knob)
constexpr int kAlsLongColumn = 8192;

// A dataset's compressed columns as the HOST sees them — what a walk's launch plan follows (fmhip_api.hip: als_plan makes it from
// a dataset): copies of cfeat / cptr, and the level schedule's offsets into a.lev_cols (NULL / 0: none) with a copy of a.lev_cols.
// The levels are taken when they hold at least 16 columns on average (FMHIP_ALS_LEVELS=0 / 1 in the environment: never / always —
// a test and measurement knob).
struct ColumnPlan {
    const int32_t *h_cfeat, *h_cptr, *h_lev_ptr, *h_lev_cols;
    int32_t n_levels;
};

hipError_t launch_als_epoch(const AlsArgs &a, const ColumnPlan &plan, hipStream_t s);

// ---- the MCMC epoch: the ALS column walk with the Gaussian conditional's draw in computeTheta's place --------------------
constexpr int kMcmcSumParts = 64;       // workgroups (= partial sums the host adds in order) per reduced quantity
// The epoch's noise of a's columns into z [(k + 1) * a.n_cols + 1] (a.n_cols = 0: the bias's alone); counter (id, group, t, stream)
// under `seed`
hipError_t launch_mcmc_noise(const AlsArgs &a, double *z, uint64_t seed, uint32_t t, hipStream_t s);
// The launches in front of the epoch's one host sync: the noise (m.sample only; z = m.z), the residuals e = yhat - y, and the sums
// the hyper-parameter draws need — sums[2 * (q * kMcmcSumParts + c)], + 1: quantity q = 0 {sum e^2, -}, q = 1 + g {sum theta,
// sum (theta - m.hyp's mu_g)^2} over group g's trained parameters.
// probit (nullable): the residual pass is k_mcmc_probit_targets' — a.y must be probit->ystar — with counter (row, attempt, t, 5).
// groups (nullable): a handle with attribute groups — m IS its McmcGroupDev; sums[] holds quantity 0 only and the groups' sums are
// k_mcmc_group_sums' (a workgroup per chunk of the plan, every partial reduced in a fixed order, no atomics), which the host adds
// in chunk order.
hipError_t launch_mcmc_begin(const AlsArgs &a, const McmcDev &m, double *z, uint64_t seed, uint32_t t, double *sums, hipStream_t s,
                             const McmcProbit *probit = nullptr, const McmcGroupSums *groups = nullptr);
// ... and behind it, with the new m.hyp on the device: the bias draw, the residuals again, q, the sweeps — launch_als_epoch's
// plan (the same environment knobs), every step a draw; with attribute groups every step looks its lambda and mu up by the
// column's group
hipError_t launch_mcmc_sweeps(const AlsArgs &a, const McmcDev &m, const ColumnPlan &plan, hipStream_t s);
hipError_t launch_mcmc_sweeps(const AlsArgs &a, const McmcGroupDev &m, const ColumnPlan &plan, hipStream_t s);
// last <- link(last), sum += last.  link: what a draw's test prediction becomes first (kLinkNone: itself)
hipError_t launch_mcmc_accumulate_link(double *last, double *sum, int64_t n_rows, const McmcLink &link, hipStream_t s);
// The test rows' predictions under the parameters t.w0 / t.w / t.v into t.e (the last draw's), then the call above over t.e: t
// holds the test set's k, n_rows, row_ptr, col, val and, as y, n_rows zeros (k_als_residual's e = yhat - 0 is the prediction exactly).
hipError_t launch_mcmc_accumulate(const AlsArgs &t, double *sum, hipStream_t s, const McmcLink &link = McmcLink{});

}  // namespace fmhip
