/*
 * dig_hip.h -- C ABI of libdig_hip.so: the MI355X (gfx950) implementation of DIGDriver's
 * mutation-rate + burden-test hot path.
 *
 * The reference (maxwellsh/DIGDriver) is pure Python and has no FFI layer; the entry points
 * below are the ones a binding for this path would need, one per vectorised reference
 * function (cited as file:line relative to the reference tree).  See INTEGRATION.md for the
 * ctypes stub a reference maintainer would add.
 *
 * Conventions
 *   - plain C symbols, caller-owned buffers, no allocation ownership crosses the boundary;
 *   - every function returns 0 on success, a negative DIG_E* code on failure; the message of
 *     the last failure on the calling thread is available from dig_last_error();
 *   - functions WITHOUT the _host suffix take DEVICE pointers valid on the current HIP device
 *     and enqueue on `stream` (a hipStream_t passed as void*; NULL = default stream); they do
 *     not synchronise and do not allocate, so they may be captured into a hipGraph;
 *   - _host twins take HOST pointers, stage through device memory on `device`, run the same
 *     kernels and synchronise before returning;
 *   - NaN/inf inputs propagate to NaN outputs exactly as the reference's numpy/scipy
 *     expressions do; there is no CPU fallback: without a HIP device every call fails.
 *   - matrices are row-major; "[E, C]" means cohort index fastest.
 */
#ifndef DIG_HIP_H
#define DIG_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DIG_OK 0
#define DIG_EINVAL (-1)   /* bad argument */
#define DIG_EHIP (-2)     /* HIP runtime error */
#define DIG_ENODEV (-3)   /* no usable gfx950 device */

#define DIG_ABI_VERSION 12  /* 2: + join, contexts, scale factors, pipeline entry points; 3: + chunked suff-stats, tile front half, RBF passes;
                             * a statistics stage leaves its worklist length in the header; 4: + dig_element_pipeline_prepare / DIG_PIPE_COMPACT_L;
                             * 5: + dig_bin_records_pack, `bin_records` argument of dig_element_pipeline; 6: + dig_count_contexts2 (2-bit genome), dig_write_tsv_host;
                             * 7: + dig_mutation_file_*_host; 8: + dig_stage_timer_*; 9: + DIG_PIPE_RECORDS, dig_element_records_*;
                             * 12 (round 6): + dig_sort_rows, dig_bh_qvalues_ragged; - dig_element_pipeline_scaled*, dig_element_pipeline_pack_counts /
                             * DIG_PIPE_PACKED_COUNTS (round 5's measured losers: tools/rejected/r05_*.patch); still 12: + dig_panel_row_keys,
                             * dig_panel_counts and their _host twins (additions); + dig_tile_sample_keys, dig_tile_sample_counts and
                             * their _host twins (additions); + dig_tile_census(_workspace), dig_sparse_tile_keys, dig_sparse_tile_test
                             * and their _host twins (additions); + dig_tile_window_test and its _host twin (additions);
                             * + dig_tile_window_sample_keys, dig_tile_window_samples and their _host twins (additions);
                             * + dig_cnv_segment_deltas, dig_cnv_window_means, their size queries and _host twins (additions);
                             * + dig_tile_window_census, dig_sparse_window_count, dig_sparse_window_test and their _host twins (additions);
                             * + dig_element_contexts_prepare / DIG_PIPE_ELEMENT_CTX (additions);
                             * + dig_element_rates_prepare, dig_element_rates_bytes / DIG_PIPE_ELEMENT_RATES (additions);
                             * + dig_element_p_prepare, dig_element_p_bytes / DIG_PIPE_ELEMENT_P (additions) */

/* dtype codes for dig_gather_bins */
#define DIG_F32 0
#define DIG_F64 1
#define DIG_I16 2
#define DIG_BF16 3

/* indices of the seven result planes written by dig_element_stats */
#define DIG_ES_EXP_SNV 0
#define DIG_ES_PVAL_SNV_BURDEN 1
#define DIG_ES_PVAL_SAMPLE_BURDEN 2
#define DIG_ES_THETA_INDEL 3
#define DIG_ES_EXP_INDEL 4
#define DIG_ES_PVAL_INDEL_BURDEN 5
#define DIG_ES_PVAL_MUT_BURDEN 6
#define DIG_ES_NPLANES 7

int dig_abi_version(void);
const char *dig_last_error(void);
/* number of HIP devices whose gcnArchName starts with "gfx950"; negative on HIP error */
int dig_device_count(void);

/* ---- negative-binomial tests (DIGDriver/sequence_model/nb_model.py) ------------------ */

/* nb_pvalue_greater_midp(k, alpha, p)  nb_model.py:271-278
 *   out[i] = 0.5 * nbinom.pmf(k[i]; alpha[i], p[i]) + betainc(k[i] + 1, alpha[i], 1 - p[i]) */
int dig_nb_midp_upper(const double *k, const double *alpha, const double *p, double *out, int64_t n, void *stream);
int dig_nb_midp_upper_host(const double *k, const double *alpha, const double *p, double *out, int64_t n, int device);

/* nb_pvalue_exact(k, alpha, p)  nb_model.py:298-314 (mu = alpha (1-p)/p) */
int dig_nb_exact(const double *k, const double *alpha, const double *p, double *out, int64_t n, void *stream);
int dig_nb_exact_host(const double *k, const double *alpha, const double *p, double *out, int64_t n, int device);

/* nb_pvalue_greater(k, alpha, p)  nb_model.py:243-256 */
int dig_nb_greater(const double *k, const double *alpha, const double *p, double *out, int64_t n, void *stream);
int dig_nb_greater_host(const double *k, const double *alpha, const double *p, double *out, int64_t n, int device);

/* nb_pvalue_midp(k, alpha, p)  nb_model.py:316-337 */
int dig_nb_midp_twosided(const double *k, const double *alpha, const double *p, double *out, int64_t n, void *stream);
int dig_nb_midp_twosided_host(const double *k, const double *alpha, const double *p, double *out, int64_t n,
                              int device);

/* Fisher combination  chi2.sf(-2 (ln p1 + ln p2), df=4)
 * DIGDriver/driver_model/transfer_tools.py:860-861,1086-1087; onthefly_tools.py:182-187 */
int dig_fisher(const double *p1, const double *p2, double *out, int64_t n, void *stream);
int dig_fisher_host(const double *p1, const double *p2, double *out, int64_t n, int device);

/* normal_params_to_gamma(mu, sigma)  nb_model.py:237-241: alpha = mu^2/sigma^2, theta = sigma^2/mu */
int dig_normal_params_to_gamma(const double *mu, const double *sigma, double *alpha, double *theta, int64_t n,
                               void *stream);
int dig_normal_params_to_gamma_host(const double *mu, const double *sigma, double *alpha, double *theta, int64_t n,
                                    int device);

/* ---- element statistics block (DIGDriver/driver_model/transfer_tools.py) ------------- *
 * One (element, cohort) pair per work item, dense [E, C]:
 *   ALPHA, THETA            load_pretrained_model            :17-19,46-48
 *   THETA *= cj[c]          transfer_element_model_with_indels :300
 *   EXP_SNV                 element_expected_muts_nb         :343-344
 *   PVAL_SNV_BURDEN         element_pvalue_burden_nb         :473-482
 *   PVAL_SAMPLE_BURDEN      element_pvalue_burden_nb_by_sample :594-615
 *   THETA_INDEL, EXP_INDEL, PVAL_INDEL_BURDEN  element_pvalue_indel :731-747
 *   PVAL_MUT_BURDEN         Fisher                           :1086-1087
 * mu_indel/sigma_indel may be NULL (= mu/sigma, the reference's indels_direct=False route,
 * genic_driver_tools.py:383-386).  pi_indel is [E] when pi_indel_per_cohort == 0, else [E, C].
 * out holds DIG_ES_NPLANES planes of E*C doubles: out[plane * E * C + e * C + c].
 * The same entry point serves the gene twins (transfer_tools.py:331-340,425-454,554-583,
 * 709-727): call it once per mutation class with that class's Pi_* / OBS_* / N_SAMP_*.
 * workspace: optional device scratch of at least dig_element_stats_workspace(E, C) bytes, 4-byte aligned.  With it the
 * rare expensive tests (k > 64 or p-value < 1e-3: lgamma + continued fraction) are compacted into a
 * queue in LDS and finished by the same kernel at the end of each workgroup (what does not fit there goes through the
 * workspace); with workspace == NULL they are resolved inline (same results, more wave divergence).
 * The function never allocates. */
int64_t dig_element_stats_workspace(int64_t E, int64_t C);
int dig_element_stats(const double *mu, const double *sigma, const double *mu_indel, const double *sigma_indel,
                      const double *pi_sum, const double *pi_indel, int pi_indel_per_cohort, const int32_t *obs_snv,
                      const int32_t *obs_samples, const int32_t *obs_indel, const double *cj, const double *cj_indel,
                      double *out, int64_t E, int64_t C, void *workspace, int64_t workspace_bytes, void *stream);
int dig_element_stats_host(const double *mu, const double *sigma, const double *mu_indel, const double *sigma_indel,
                           const double *pi_sum, const double *pi_indel, int pi_indel_per_cohort,
                           const int32_t *obs_snv, const int32_t *obs_samples, const int32_t *obs_indel,
                           const double *cj, const double *cj_indel, double *out, int64_t E, int64_t C, int device);

/* ---- per-element accumulation (DIGDriver/sequence_model/genic_driver_tools.py) ------- *
 * nonc_model :300-431 (n_class = 1), genic_model :31-203 (n_class = 4: silent, missense,
 * nonsense, splice columns of L_data), tiled_nonc_model :599-690 (one bin per element), and the
 * loop body of DIG_onthefly (driver_model/onthefly_tools.py:109-164), for all C cohorts at once:
 *   MU = sum Y_PRED, SIGMA = sqrt(sum STD^2), R_OBS = sum Y_TRUE, FLAG = OR of FLAG over the
 *   element's overlapped bins (the reference adds numpy bools: logical OR, result 0/1)
 *                                                     get_region_params_direct :258-272
 *   region_counts = sum of the bins' 64 context counts, each repeated x3, reverse-complement
 *   permuted for '-' strand elements                  sequence_tools.py:630-634
 *   t_pi = d_pr / sum(region_counts * d_pr);  P = sum(t_pi * L)        :361-367
 *   R_SIZE = int(sum(region_counts)/3); ELT_SIZE = int(sum(L)/3); P_INDEL = ELT_SIZE/R_SIZE :375-381
 *   (gene_length != NULL: P_INDEL = gene_length / R_SIZE, genic_driver_tools.py:158-159)
 * Inputs (device): bin_mu, bin_std f64 [N, C]; bin_y i32 [N, C]; bin_flag u8 [N, C];
 *   bin_ctx i32 [N, 64] (contexts in sorted ACGT^3 order); ov_ptr i64 [E+1], ov_idx i32 [nnz]
 *   (CSR of overlapped bin rows, see dig_ideal_overlaps_host); L i32 [E, n_class, 192] in sorted
 *   substitution order ("XYZ>XaZ"); strand_minus u8 [E]; d_pr f64 [C, 192] = FREQ re-indexed by
 *   sorted substitution string (genic_driver_tools.py:321-325).
 * Outputs (device): MU, SIGMA f64 [E, C]; R_OBS, FLAG i32 [E, C]; P f64 [E, n_class, C];
 *   R_SIZE, ELT_SIZE i32 [E]; P_INDEL f64 [E].
 * workspace: device scratch of at least dig_accumulate_workspace(E, C) bytes, 256-byte aligned
 *   (strand-permuted context counts per element + transposed parameter tables).  With
 *   workspace == NULL a slower single-kernel LDS variant runs.  The function never allocates. */
int64_t dig_accumulate_workspace(int64_t E, int64_t C);
int dig_accumulate_elements(const double *bin_mu, const double *bin_std, const int32_t *bin_y,
                            const uint8_t *bin_flag, const int32_t *bin_ctx, const int64_t *ov_ptr,
                            const int32_t *ov_idx, const int32_t *L, int n_class, const uint8_t *strand_minus,
                            const int32_t *gene_length, const double *d_pr, double *MU, double *SIGMA,
                            int32_t *R_OBS, int32_t *FLAG, double *P, int32_t *R_SIZE, int32_t *ELT_SIZE,
                            double *P_INDEL, int64_t N, int64_t E, int64_t C, void *workspace,
                            int64_t workspace_bytes, void *stream);
int dig_accumulate_elements_host(const double *bin_mu, const double *bin_std, const int32_t *bin_y,
                                 const uint8_t *bin_flag, const int32_t *bin_ctx, const int64_t *ov_ptr,
                                 const int32_t *ov_idx, const int32_t *L, int n_class, const uint8_t *strand_minus,
                                 const int32_t *gene_length, const double *d_pr, double *MU, double *SIGMA,
                                 int32_t *R_OBS, int32_t *FLAG, double *P, int32_t *R_SIZE, int32_t *ELT_SIZE,
                                 double *P_INDEL, int64_t N, int64_t E, int64_t C, int device);

/* ---- accumulation + statistics block as one operation --------------------------------------- *
 * dig_element_pipeline == dig_accumulate_elements (n_class = 1) followed by dig_element_stats(MU, SIGMA, NULL, NULL,
 * P, P_INDEL [E], obs..., cj, cj_indel, out): the elementDriver / tiledModel route from bin tables to p-values
 * (genic_driver_tools.py:300-431 then transfer_tools.py:1069-1087).  One fusion across the two: MU / SIGMA / R_OBS /
 * FLAG are summed inside the statistics streaming kernel instead of being written by one kernel and read back by
 * the next.  All outputs of both operations are written; results are bit-identical to the two separate calls.
 * stages: DIG_PIPE_ALL, or the stages as separate calls in the order CONTEXTS, DOT, STATISTICS on the same workspace
 *   (only STATISTICS reads cj / cj_indel / obs_*: a caller can form the scale factors on another stream meanwhile,
 *   e.g. beside the MFMA-bound DOT kernel, and make `stream` wait for them before the statistics call).
 * workspace: dig_element_pipeline_workspace(E, C) bytes (0 = not available: E * C >= 2^32 - 1), 256-byte aligned. */
#define DIG_PIPE_CONTEXTS 1   /* acc_region_kernel: context rows, parameter table, R_SIZE */
#define DIG_PIPE_DOT 2        /* acc_dot_mfma_kernel: P, ELT_SIZE, P_INDEL */
#define DIG_PIPE_ACCUMULATE 3
#define DIG_PIPE_STATISTICS 4 /* MU, SIGMA, R_OBS, FLAG and the seven statistics planes */
#define DIG_PIPE_ALL 7
/* A call WITHOUT the CONTEXTS stage clears the worklist header of the statistics stage with a memset node of its own.
 * OR this flag into `stages` to skip that node when the caller knows the header is clear: after a CONTEXTS call on the
 * same workspace with no STATISTICS call since (a statistics stage leaves counts in the header: dword 2 the pairs it
 * finished from the global worklist, dword 3 the pairs the fused stream pass finished from its workgroups' LDS queues). */
#define DIG_PIPE_WORKLIST_CLEAN 8
/* Context-repeated L (ABI 4).  The reference builds the L_counts of every element / tile / on-the-fly region as its 64
 * trinucleotide context counts, each written to the three substitutions of that context (sequence_tools.py:560-564): then
 * sum(t_pi * L) runs over the same 64 per-context sums of d_pr as the denominator sum(region_counts * d_pr), and contexts +
 * dot become ONE kernel with half the matrix work (acc_dot_ctx_kernel; no acc_region_kernel, no parameter-table pass).
 *   dig_element_pipeline_prepare  PLAN TIME, once per element set: checks L[e, 3 j] == L[e, 3 j + 1] == L[e, 3 j + 2] for
 *       every element and context on the device, writes the compact [E, 64] counts into `workspace`, waits for `stream`
 *       and reports *compact_ok (host int) = 1 / 0.  Genic (n_class = 4) and --f-sites sets give 0.
 *   DIG_PIPE_COMPACT_L  OR into `stages` of dig_element_pipeline calls on a workspace prepared with compact_ok = 1 for
 *       this very L.  The CONTEXTS stage is then empty; the DOT stage is the fused kernel and clears the worklist header.
 *       Denominators are bit-identical to the general form, numerators differ by the rounding of a regrouped sum (P within
 *       a few ulp; tests/test_gpu_parity.py).  Without the flag the general K = 256 form runs, as before. */
#define DIG_PIPE_COMPACT_L 16
/* Element context rows as a plan-time product (compact form only).  The region counts of an element,
 *     elt_ctx[e, j] = sum over the element's bins of bin_ctx[bin, j]            ('+' strand)
 *                   = sum over the element's bins of bin_ctx[bin, revcomp(j)]   ('-' strand),
 *     revcomp(16 t + 4 k + u) = 16 (3 - u) + 4 (3 - k) + (3 - t)                (sequence_tools.py:630-634),
 * depend on bin_ctx, ov_ptr, ov_idx and strand_minus only -- the genome's bins and the element set, the same for every cohort
 * and every call -- and are integers, so forming them once changes no bit of any output.
 *   dig_element_contexts_prepare  PLAN TIME, once per element set (again after bin_ctx / ov_* / strand_minus changed): writes
 *       the [E, 64] int32 table (caller-owned, 256-byte aligned; the table the general form's CONTEXTS stage leaves at the
 *       start of its workspace).  An element without bins gets zeros.  Enqueued on `stream`; nothing is waited for.
 *   DIG_PIPE_ELEMENT_CTX  OR into `stages` together with DIG_PIPE_COMPACT_L (alone: DIG_EINVAL): the `bin_ctx` argument of
 *       dig_element_pipeline is then that table, and the DOT stage streams it like the compact L (no CSR walk, no gather,
 *       no strand selects in acc_dot_ctx_kernel); the STATISTICS stage still reads ov_ptr / ov_idx (unless DIG_PIPE_ELEMENT_RATES).  Same bits as without. */
#define DIG_PIPE_ELEMENT_CTX 64
int dig_element_contexts_prepare(const int32_t *bin_ctx, const int64_t *ov_ptr, const int32_t *ov_idx,
                                 const uint8_t *strand_minus, int64_t N, int64_t E, int32_t *elt_ctx, void *stream);
/* Record-major outputs of the statistics stage (ABI 9).  The stage has eleven outputs per (element, cohort) pair -- the seven
 * planes of dig_element_stats and MU, SIGMA, R_OBS, FLAG of the accumulation (transfer_tools.py:343-344,473-482,594-615,
 * 731-747,1086-1087; genic_driver_tools.py:404-417) -- i.e. eleven store streams whose tile starts fall on odd 8-byte
 * boundaries (E * C is rarely a multiple of 16).  With DIG_PIPE_RECORDS in `stages`, `out` is instead TILE-BLOCKED RECORDS:
 *     double out[ceil(E * C / 64)][DIG_REC_DOUBLES / 2][64][2]      (256-byte aligned)
 * the ten fields of pair i = e * C + c -- [DIG_ES_EXP_SNV .. DIG_ES_PVAL_MUT_BURDEN] the seven statistics in plane order,
 * [DIG_REC_MU], [DIG_REC_SIGMA], and at [DIG_REC_ROBS_FLAG] the two int32 R_OBS (low word) and FLAG (high word) -- live in
 * block i / 64: field f at out[i / 64][f / 2][i % 64][f % 2].  A lane of the kernel writes its ten fields as five 16-byte
 * pieces; a wave's five store instructions write 1 KB each, ONE aligned 5 120-byte run per 64-pair tile from one base
 * address, and nothing passes through LDS.  MU / SIGMA / R_OBS / FLAG arguments are not written (may be NULL); the lanes
 * past E * C of the last block are scratch.  Needs `bin_records`.  Values are bit-identical to the plane form.
 * dig_element_records_unpack turns the blocks into the plane form (out7 [7, E, C], MU, SIGMA [E, C] doubles, R_OBS, FLAG
 * [E, C] int32; any destination may be NULL; cohort_major: every plane as [C, E]). */
#define DIG_PIPE_RECORDS 32
#define DIG_REC_DOUBLES 10
#define DIG_REC_MU 7
#define DIG_REC_SIGMA 8
#define DIG_REC_ROBS_FLAG 9
int64_t dig_element_records_bytes(int64_t E, int64_t C);
int dig_element_records_unpack(const double *records, int64_t E, int64_t C, double *out7, double *MU, double *SIGMA,
                               int32_t *R_OBS, int32_t *FLAG, int cohort_major, void *stream);
int64_t dig_element_pipeline_workspace(int64_t E, int64_t C);
/* Stage timers (ABI 8; measurement only).  How long did the dot kernel / the statistics kernel of a dig_element_pipeline call
 * run?  Two events around a stage on the stream measure more than the kernel (each is a packet of its own: ~6 us, and the
 * packets change what runs beside the kernel on other streams).  A timer armed for DIG_PIPE_DOT or DIG_PIPE_STATISTICS makes
 * the NEXT launch of that stage's kernel by the calling thread record its own begin and end (hipExtLaunchKernelGGL: the
 * times of the dispatch itself, what rocprofv3's kernel trace shows; nothing is added to the stream).  dig_stage_timer_read
 * waits for that kernel and returns its duration in milliseconds; DIG_EINVAL if no such launch followed the arming. */
int dig_stage_timer_create(void **timer);
int dig_stage_timer_arm(void *timer, int stage);
int dig_stage_timer_read(void *timer, double *ms);
/* what the timer reads for a kernel that does nothing (one wave, launched here on `stream`): the part of a reading that is dispatch, not kernel */
int dig_stage_timer_selftest(void *timer, void *stream);
int dig_stage_timer_destroy(void *timer);
int dig_element_pipeline_prepare(const int32_t *L, int64_t E, int64_t C, void *workspace, int64_t workspace_bytes,
                                 int *compact_ok, void *stream);
/* host twin: all pointers in host memory; stages the arrays, checks L (the compact form runs when it repeats), runs
 * DIG_PIPE_ALL on the null stream and copies every output of accumulation and statistics back */
int dig_element_pipeline_host(const double *bin_mu, const double *bin_std, const int32_t *bin_y, const uint8_t *bin_flag,
                              const int32_t *bin_ctx, const int64_t *ov_ptr, const int32_t *ov_idx, const int32_t *L,
                              const uint8_t *strand_minus, const int32_t *gene_length, const double *d_pr,
                              const int32_t *obs_snv, const int32_t *obs_samples, const int32_t *obs_indel, const double *cj,
                              const double *cj_indel, double *MU, double *SIGMA, int32_t *R_OBS, int32_t *FLAG, double *P,
                              int32_t *R_SIZE, int32_t *ELT_SIZE, double *P_INDEL, double *out, int64_t N, int64_t E, int64_t C,
                              int device);
/* Packed bin records (ABI 5), PLAN TIME, once per set of bin tables: the statistics stage gathers Y_PRED, STD, Y_TRUE and
 * FLAG of every bin an element overlaps (get_region_params_direct, genic_driver_tools.py:258-272) -- four arrays, four
 * random row segments per bin.  dig_bin_records_pack rewrites them as {Y_PRED, STD^2} pairs (16 bytes) and
 * Y_TRUE | (FLAG != 0) << 31 (4 bytes) per (bin, cohort): two gathers per bin, the square of :266 taken once.  Pass the
 * records as `bin_records` of dig_element_pipeline (NULL: the four tables are read as before; they stay required either
 * way).  Same bits as without.  The call waits for `stream`; Y_TRUE must be >= 0.  Repack when a table changes. */
int64_t dig_bin_records_bytes(int64_t N, int64_t C);
int dig_bin_records_pack(const double *bin_mu, const double *bin_std, const int32_t *bin_y, const uint8_t *bin_flag, int64_t N,
                         int64_t C, void *records, int64_t records_bytes, void *stream);
/* Element rate sums as a plan-time product (packed bin records only).  MU = sum Y_PRED, SIGMA = sqrt(sum STD^2), R_OBS = sum
 * Y_TRUE and FLAG = OR of FLAG over a pair's bins (get_region_params_direct, genic_driver_tools.py:258-272) depend on the bin
 * records and on ov_ptr / ov_idx only -- not on the scale factors, the observed counts or P -- so a caller that runs the
 * same tables many times forms them once.  The additions are those of the statistics kernel in its order (from 0.0, the
 * element's bins first to last) and the square root is the same code: the four outputs keep their bits.
 *   dig_element_rates_prepare  PLAN TIME, once per set of records and overlaps (again after dig_bin_records_pack or a change
 *       of ov_ptr / ov_idx): writes the table -- per 64-pair tile 64 x {double MU, SIGMA} then 64 x {int32 R_OBS, FLAG}, 1 536
 *       bytes a tile, pair i = e * C + c in tile i / 64 at lane i % 64; the lanes past E * C of the last tile repeat the last
 *       pair -- into `rates` (caller-owned, 256-byte aligned, at least dig_element_rates_bytes(E, C) bytes).  An element
 *       without bins gives 0, 0, 0, 0.  Enqueued on `stream`; nothing is waited for.
 *   DIG_PIPE_ELEMENT_RATES  OR into `stages` of dig_element_pipeline calls that pass `bin_records` (without: DIG_EINVAL): the
 *       `bin_mu` argument is then that table, and the STATISTICS stage streams it with its other per-pair inputs (no CSR
 *       walk, no index loads, no gathers, no loop over further bins, no sqrt in element_stats_stream_fused_kernel); it reads
 *       neither the bin tables nor the records nor ov_ptr / ov_idx.  MU / SIGMA / R_OBS / FLAG are still written by every
 *       call.  Same bits as without.  A caller that runs its tables ONCE gains nothing: the table is an extra write and read
 *       of 24 bytes per pair. */
#define DIG_PIPE_ELEMENT_RATES 128
int64_t dig_element_rates_bytes(int64_t E, int64_t C);
int dig_element_rates_prepare(const void *bin_records, const int64_t *ov_ptr, const int32_t *ov_idx, int64_t N, int64_t E,
                              int64_t C, void *rates, int64_t rates_bytes, void *stream);
/* P as a plan-time product (either form of the accumulation).  P = sum L d_pr / sum region_counts d_pr, R_SIZE, ELT_SIZE and
 * P_INDEL (genic_driver_tools.py:404-417: the reference stores P_SUM with MU and SIGMA in the pretrained element table, and
 * the driver, transfer_tools.py:281-344, only reads it) depend on L, the context rows, gene_length and d_pr only -- not on
 * the scale factors or the observed counts -- so a caller that runs the same element set and cohorts many times forms them
 * once and has every later call copy them.
 *   dig_element_p_prepare  PLAN TIME, after ONE accumulation call of whatever form (compact, planned contexts, general K =
 *       256, C > 48 in chunks): bit copies of that call's four outputs go into `table` (caller-owned, 256-byte aligned, at
 *       least dig_element_p_bytes(E, C) bytes): P [E C] f64 | P_INDEL [E] f64 | R_SIZE [E] int32 | ELT_SIZE [E] int32, every
 *       section starting on a 256-byte boundary.  The table holds that form's bits, the NaN / inf of zero denominators
 *       included.  Enqueued on `stream`; nothing is waited for.  Again after L, d_pr, gene_length, bin_ctx, ov_* or
 *       strand_minus changed.
 *   DIG_PIPE_ELEMENT_P  OR into `stages` of dig_element_pipeline calls: the `d_pr` argument is then that table (NULL or
 *       misaligned: DIG_EINVAL).  The CONTEXTS stage enqueues nothing; the DOT stage is ONE launch of element_p_stream_kernel
 *       whatever C is, which writes P, R_SIZE, ELT_SIZE and P_INDEL from the table into the caller's outputs (8 bytes in and
 *       out per pair, no matrix work) and clears the worklist header; a DIG_PIPE_DOT stage timer reads that kernel.  The
 *       accumulation stages read neither bin_ctx, ov_ptr / ov_idx, L, strand_minus nor gene_length; the STATISTICS stage is
 *       unchanged and reads the caller's P / P_INDEL.  All four outputs are still written by every call.  The host twin and a
 *       caller that runs its tables ONCE keep the live form: for them the table is an extra write and read. */
#define DIG_PIPE_ELEMENT_P 256
int64_t dig_element_p_bytes(int64_t E, int64_t C);
int dig_element_p_prepare(const double *P, const int32_t *R_SIZE, const int32_t *ELT_SIZE, const double *P_INDEL, int64_t E,
                          int64_t C, void *table, int64_t table_bytes, void *stream);
int dig_element_pipeline(const double *bin_mu, const double *bin_std, const int32_t *bin_y, const uint8_t *bin_flag,
                         const int32_t *bin_ctx, const int64_t *ov_ptr, const int32_t *ov_idx, const int32_t *L,
                         const uint8_t *strand_minus, const int32_t *gene_length, const double *d_pr,
                         const int32_t *obs_snv, const int32_t *obs_samples, const int32_t *obs_indel, const double *cj,
                         const double *cj_indel, double *MU, double *SIGMA, int32_t *R_OBS, int32_t *FLAG, double *P,
                         int32_t *R_SIZE, int32_t *ELT_SIZE, double *P_INDEL, double *out, int64_t N, int64_t E, int64_t C,
                         const void *bin_records, int stages, void *workspace, int64_t workspace_bytes, void *stream);
/* ---- the gene route's statistics block as one launch (ABI 4) -------------------------------- *
 * gene_expected_muts_nb :331-340, gene_pvalue_burden_nb :394-456, gene_pvalue_burden_nb_by_sample :554-583,
 * gene_pvalue_indel :709-729 and the Fisher combination :860-861 of driver_model/transfer_tools.py, for G genes x C cohorts;
 * classes SYN, MIS, NONS, SPL, TRUNC = NONS + SPL, NONSYN = MIS + TRUNC.
 *   mu, sigma f64 [G, C] (ALPHA, THETA = normal_params_to_gamma; THETA *= cj[c]); mu_indel, sigma_indel: the indel pair or NULL
 *   pi f64 [G, n_pi, C]: n_pi = 6 (Pi_SYN .. Pi_NONSYN as load_pretrained_model hands them) or 4 (P_SILENT, P_MIS, P_NONS,
 *       P_SPLICE straight from dig_accumulate_elements(n_class = 4): TRUNC and NONSYN are added here)
 *   pi_indel f64 [G] or [G, C]; obs i32 [G, 5, C] = OBS_SYN, MIS, NONS, SPL, INDEL (TRUNC / NONSYN are added here);
 *   n_samp i32 [G, 6, C] = N_SAMP_c (distinct samples per class); cj, t_indel f64 [C] (t_indel: the indel calibration of
 *       :720-721, formed by the caller over its null gene set); with_indel = 0 leaves the four indel planes NaN.
 *   out f64 [22, G, C]: EXP_c x 6, PVAL_c_BURDEN x 6, PVAL_c_BURDEN_SAMPLE x 6, THETA_INDEL, EXP_INDEL, PVAL_INDEL_BURDEN,
 *       PVAL_MUT_BURDEN (Fisher of PVAL_TRUNC_BURDEN and PVAL_INDEL_BURDEN).
 * dig_gene_pipeline == dig_accumulate_elements(n_class = 4, gene_length) followed by dig_gene_stats(MU, SIGMA, NULL, NULL, P, 4,
 *   P_INDEL [G], ...): genic_model (genic_driver_tools.py:31-203) to p-values in one call; workspace as dig_accumulate_elements. */
int dig_gene_stats(const double *mu, const double *sigma, const double *mu_indel, const double *sigma_indel, const double *pi,
                   int n_pi, const double *pi_indel, int pi_indel_per_cohort, const int32_t *obs, const int32_t *n_samp,
                   const double *cj, const double *t_indel, int with_indel, double *out, int64_t G, int64_t C, void *stream);
int dig_gene_stats_host(const double *mu, const double *sigma, const double *mu_indel, const double *sigma_indel,
                        const double *pi, int n_pi, const double *pi_indel, int pi_indel_per_cohort, const int32_t *obs,
                        const int32_t *n_samp, const double *cj, const double *t_indel, int with_indel, double *out, int64_t G,
                        int64_t C, int device);
int dig_gene_pipeline(const double *bin_mu, const double *bin_std, const int32_t *bin_y, const uint8_t *bin_flag,
                      const int32_t *bin_ctx, const int64_t *ov_ptr, const int32_t *ov_idx, const int32_t *L,
                      const uint8_t *strand_minus, const int32_t *gene_length, const double *d_pr, const int32_t *obs,
                      const int32_t *n_samp, const double *cj, const double *t_indel, int with_indel, double *MU, double *SIGMA,
                      int32_t *R_OBS, int32_t *FLAG, double *P, int32_t *R_SIZE, int32_t *ELT_SIZE, double *P_INDEL, double *out,
                      int64_t N, int64_t G, int64_t C, void *workspace, int64_t workspace_bytes, void *stream);
int dig_gene_pipeline_host(const double *bin_mu, const double *bin_std, const int32_t *bin_y, const uint8_t *bin_flag,
                           const int32_t *bin_ctx, const int64_t *ov_ptr, const int32_t *ov_idx, const int32_t *L,
                           const uint8_t *strand_minus, const int32_t *gene_length, const double *d_pr, const int32_t *obs,
                           const int32_t *n_samp, const double *cj, const double *t_indel, int with_indel, double *MU,
                           double *SIGMA, int32_t *R_OBS, int32_t *FLAG, double *P, int32_t *R_SIZE, int32_t *ELT_SIZE,
                           double *P_INDEL, double *out, int64_t N, int64_t G, int64_t C, int device);

/* ---- the gene route's dN/dS correction and selection tests as one launch (additive: the ABI version stays) --- *
 * gene_expected_muts_dnds :363-392 (_mle_t, _mrfold_factor :1264-1277), gene_pvalue_burden_dnds :617-655, gene_pvalue_sel_nb
 * :657-676 (_llr_test_nb :1172-1213), gene_pvalue_sel_gamma :749-765 (_llr_test_gamma_poiss :1215-1252) and
 * selection_coefficient :1280-1292 of driver_model/transfer_tools.py, for G genes x C cohorts; classes as dig_gene_stats.
 *   alpha, theta f64 [G, C]: the frame's ALPHA and THETA columns (THETA already scaled by the cohort factor);
 *   pi f64 [G, n_pi, C], n_pi = 6 or 4 as dig_gene_stats; obs i32 [G, 5, C] = OBS_SYN, MIS, NONS, SPL, INDEL (INDEL unused).
 *   out f64 [DIG_SEL_NPLANES = 34, G, C]:
 *      0- 1  T_SYN, MRFOLD                     T_SYN = _mle_t(OBS_SYN, 1, ALPHA, THETA Pi_SYN), MRFOLD = max(1e-10, T_SYN / EXP_SYN)
 *      2- 7  EXP_c_ML                          c = SYN, MIS, NONS, SPL, TRUNC, NONSYN: EXP_c MRFOLD
 *      8-13  PVAL_c_BURDEN_DNDS                mid-p burden test at 1 / (EXP_c_ML / ALPHA + 1)
 *     14-17  PVAL_{SYN,MIS,TRUNC,NONSYN}_SEL_NB   likelihood-ratio tests under the NB model (df 1, 1, 1, 2)
 *     18-21  PVAL_{SYN,MIS,NONS,NONSYN}_SEL_PG    the same under the Gamma-Poisson model
 *     22-27  SEL_c                             (OBS_c + 1e-16) / (EXP_c + 1e-16)
 *     28-33  PVAL_c_SEL                        df 1 likelihood ratio between THETA Pi_c and THETA Pi_c SEL_c
 *   Both maxima are Python's max(a, b) (a unless b > a): a NaN T_SYN / EXP_SYN gives MRFOLD = 1e-10.  Otherwise NaN in, NaN out,
 *   and NaN wherever the reference's sums of log-likelihoods hold -inf on both sides. */
#define DIG_SEL_NPLANES 34
int dig_gene_selection(const double *alpha, const double *theta, const double *pi, int n_pi, const int32_t *obs, double *out,
                       int64_t G, int64_t C, void *stream);
int dig_gene_selection_host(const double *alpha, const double *theta, const double *pi, int n_pi, const int32_t *obs, double *out,
                            int64_t G, int64_t C, int device);

/* ---- the gene route's observed counts for many cohorts (additive: the ABI version stays) ---------------------- *
 * filter_hypermut_samples + mutations_per_gene (mutation_tools.py:293-304,329-361), the N_SAMP_* columns of transfer_gene_model
 * (transfer_tools.py:196-270) and the synonymous row count of the scale factor (:809-823) for the coding rows of C cohorts against
 * one gene index of G rows.  A row is (gene id, sample id dense per cohort, class, cohort): gene 0 .. G - 1 = the model's rows, G =
 * a gene outside the model, G + 1 = TP53 when the model has no TP53 row; class 0 Synonymous, 1 Missense, 2 Nonsense,
 * 3 Essential_Splice, 4 INDEL, 5 anything else.  sample_off i64 [C + 1]: a cohort's first global sample (0 first, n_samples last).
 *   dig_gene_row_keys: keys i64 [n], key = (cohort (G + 2) + gene) << (sb + 3) | global sample << 3 | class with sb the bits of
 *     n_samples - 1 (DIG_EINVAL when the fields do not fit 63 bits), and sample_total i32 [n_samples] = rows per sample.  A row
 *     outside the tables gets key -1 and is counted nowhere (the host twin refuses it).
 *   The caller sorts the keys ascending (as for dig_bh_qvalues_sorted).
 *   dig_gene_counts, from the sorted keys: a sample with sample_total > max_muts_per_sample (a double, the reference's `>`) is
 *     blacklisted [n_samples] u8 and none of its rows count.  Of the others:
 *       obs i32 [G, 5, C]     rows per (gene, class 0 .. 4, cohort), each (gene, sample, class) group clipped to
 *                             max_muts_per_gene_per_sample as the reference clips: summed as numbers, then cast to int
 *       n_samp i32 [G, 6, C]  distinct (gene, sample) pairs with a row of class SYN, MIS, NONS, SPL, TRUNC = {NONS, SPL}, NONSYN =
 *                             {MIS, NONS, SPL} (unclipped); the layouts dig_gene_stats reads
 *       extra i32 [G, 2, C]   the same for INDEL (N_SAMP_INDEL), and for a row of any class (a gene with 0 here has no row in the
 *                             reference's count table: its merge turns the cohort's OBS_* columns into floats)
 *       n_syn i64 [C]         class-0 rows of every gene but `tp53` (a gene id; G + 1 when the model has no TP53), genes outside
 *                             the model included, unclipped
 *     scratch: i32 [G, 5, C] of device memory.  Every output is zeroed by the call; integer atomics, so order-independent. */
int dig_gene_row_keys(const int32_t *gene, const int32_t *sample, const uint8_t *annot, const int32_t *cohort, const int64_t *sample_off,
                      int64_t n, int64_t G, int64_t C, int64_t n_samples, int64_t *keys, int32_t *sample_total, void *stream);
int dig_gene_row_keys_host(const int32_t *gene, const int32_t *sample, const uint8_t *annot, const int32_t *cohort,
                           const int64_t *sample_off, int64_t n, int64_t G, int64_t C, int64_t n_samples, int64_t *keys,
                           int32_t *sample_total, int device);
int dig_gene_counts(const int64_t *keys_sorted, int64_t n, const int32_t *sample_total, int64_t n_samples, double max_muts_per_sample,
                    double max_muts_per_gene_per_sample, int64_t tp53, int64_t G, int64_t C, int32_t *obs, int32_t *n_samp,
                    int32_t *extra, int64_t *n_syn, uint8_t *blacklisted, int32_t *scratch, void *stream);
int dig_gene_counts_host(const int64_t *keys_sorted, int64_t n, const int32_t *sample_total, int64_t n_samples,
                         double max_muts_per_sample, double max_muts_per_gene_per_sample, int64_t tp53, int64_t G, int64_t C,
                         int32_t *obs, int32_t *n_samp, int32_t *extra, int64_t *n_syn, uint8_t *blacklisted, int device);

/* ---- the target route's panel counts for many cohorts (additive: the ABI version stays) ------------------------ *
 * What CohortRun.panel_scale (transfer_tools.py:905-935) and DigPretrain.py countMutations (:103-177) count per sequencing panel, for
 * the rows of C cohorts and P <= 32 panels at once.  A row is (label, sample id dense per cohort, class, cohort): label 0 .. L - 1 =
 * the place of the row's GENE in a table of L genes (the union of the panels), L = in no panel; label_mask u32 [L]: bit p set when the
 * gene is in panel p (bits from P on are ignored); class 0 Synonymous, 1 Missense, 2 Nonsense, 3 Essential_Splice, 4 INDEL, 5 any
 * other label, 6 Noncoding.  sample_off i64 [C + 1] as for dig_gene_row_keys; skip u8 [n_samples] or NULL: non-zero = a blacklisted
 * sample, whose rows count nowhere.  L within [1, 2^31), C < 2^31.
 *   dig_panel_row_keys: n_cds i64 [C] = rows of class != 6, and keys i64 [n]: a row of class 1, 2, 4 or 5 whose label has a panel
 *     gets key = global sample << lb | label with lb the bits of L - 1 (DIG_EINVAL, before any launch, when the two fields do not
 *     fit 63 bits); every other row, and a row outside the tables (the host twin refuses that one), gets key -1.
 *   The caller sorts the keys ascending (as for dig_gene_counts).
 *   dig_panel_counts, from the sorted keys, i64 [C, P] each: n_mut = counted rows per (cohort, panel), n_pairs = distinct (label,
 *     sample) pairs, n_sample = distinct samples with a counted row in the panel.  Distinct samples: the head of a sample's first
 *     (sample, label) run walks that sample's label runs and ORs their masks -- no scratch buffer, no size query, no second kernel.
 *   Every output is zeroed by the call; integer atomics, so order-independent.  Alignment: that of the element types (8 bytes for
 *   keys, sample_off and the outputs, 4 for label, sample, cohort and label_mask, 1 for annot and skip). */
int dig_panel_row_keys(const int32_t *label, const int32_t *sample, const uint8_t *annot, const int32_t *cohort, const int64_t *sample_off,
                       const uint8_t *skip, const uint32_t *label_mask, int64_t n, int64_t L, int64_t P, int64_t C, int64_t n_samples,
                       int64_t *keys, int64_t *n_cds, void *stream);
int dig_panel_row_keys_host(const int32_t *label, const int32_t *sample, const uint8_t *annot, const int32_t *cohort,
                            const int64_t *sample_off, const uint8_t *skip, const uint32_t *label_mask, int64_t n, int64_t L, int64_t P,
                            int64_t C, int64_t n_samples, int64_t *keys, int64_t *n_cds, int device);
int dig_panel_counts(const int64_t *keys_sorted, int64_t n, const uint32_t *label_mask, const int64_t *sample_off, int64_t L, int64_t P,
                     int64_t C, int64_t n_samples, int64_t *n_mut, int64_t *n_pairs, int64_t *n_sample, void *stream);
int dig_panel_counts_host(const int64_t *keys_sorted, int64_t n, const uint32_t *label_mask, const int64_t *sample_off, int64_t L,
                          int64_t P, int64_t C, int64_t n_samples, int64_t *n_mut, int64_t *n_pairs, int64_t *n_sample, int device);

/* ---- the region model's training labels for many cohorts (additive: the ABI version stays) -------------------- *
 * scripts/DataExtractor.py:525-572 add_objectives, the SNV branch (--cnv: dig_cnv_* below): mutation counts per window of the data container's `idx`.  The
 * (mutation row, window) pairs come from dig_overlap_join_count/fill with the N windows as one-block elements and the rows of all C
 * cohorts as mutations.  A row carries its global sample (sample_off i64 [C + 1]: a cohort's first global sample, 0 first, n_samples
 * last), its mutation id -- dense ids of the distinct (CHROM, START, END, REF, ALT) of its cohort, all below n_uid: with the sample
 * and the window the identity tabulate_muts_per_sample_per_element(drop_duplicates=True) de-duplicates on, mutation_tools.py:208 --
 * and its indel byte (ANNOT == 'INDEL').
 *   dig_window_pair_keys: keys i64 [n_pairs], key = global sample << (wb + 1 + ub) | window << (1 + ub) | indel << ub | mutation id,
 *     ub / wb the bits of n_uid - 1 / N - 1 (DIG_EINVAL when the fields do not fit 63 bits).  The window of a pair is
 *     blk_window[pair_blk] (blk_window i32 [n_blk]; NULL: the block row itself).  A pair outside the tables gets key -1 and is counted
 *     nowhere (the host twin refuses it).
 *   The caller sorts the keys ascending (as for dig_gene_counts).
 *   dig_window_sample_hits, from the sorted keys: hits i32 [n_samples] = the distinct windows a sample has a row in, SNV or INDEL --
 *     what SAMPLE.value_counts() is on the reference's (window, sample) frame (filter_samples_by_stdev, filter_hypermut_samples,
 *     mutation_tools.py:293-316).  The caller forms keep u8 [n_samples] from it.
 *   dig_window_objectives, from the same keys: labels f64 [N, C] = per window and cohort the number of DISTINCT keys with a clear indel
 *     bit among the kept samples (DataExtractor.py:559-562).  scratch: i32 [N, C] of device memory.
 * Every output is zeroed by its call; integer atomics, one per run of lanes with one destination, so order-independent. */
int dig_window_pair_keys(const int32_t *pair_row, const int32_t *pair_blk, int64_t n_pairs, const int32_t *blk_window, int64_t n_blk,
                         const int32_t *row_sample, const int32_t *row_uid, const uint8_t *row_indel, int64_t n_rows,
                         int64_t n_samples, int64_t N, int64_t n_uid, int64_t *keys, void *stream);
int dig_window_pair_keys_host(const int32_t *pair_row, const int32_t *pair_blk, int64_t n_pairs, const int32_t *blk_window,
                              int64_t n_blk, const int32_t *row_sample, const int32_t *row_uid, const uint8_t *row_indel,
                              int64_t n_rows, int64_t n_samples, int64_t N, int64_t n_uid, int64_t *keys, int device);
int dig_window_sample_hits(const int64_t *keys_sorted, int64_t n_pairs, int64_t n_samples, int64_t N, int64_t n_uid, int32_t *hits,
                           void *stream);
int dig_window_sample_hits_host(const int64_t *keys_sorted, int64_t n_pairs, int64_t n_samples, int64_t N, int64_t n_uid,
                                int32_t *hits, int device);
int dig_window_objectives(const int64_t *keys_sorted, int64_t n_pairs, const uint8_t *keep, const int64_t *sample_off,
                          int64_t n_samples, int64_t N, int64_t C, int64_t n_uid, double *labels, int32_t *scratch, void *stream);
int dig_window_objectives_host(const int64_t *keys_sorted, int64_t n_pairs, const uint8_t *keep, const int64_t *sample_off,
                               int64_t n_samples, int64_t N, int64_t C, int64_t n_uid, double *labels, int device);

/* ---- the region model's copy-number training labels for many cohorts (additive: the ABI version stays) -------- *
 * scripts/DataExtractor.py:100-154,535-539 add_objectives --cnv: per window [s, s + W) of the data container's `idx` the mean over its
 * W positions of three per-base tracks built from a cohort's copy-number segments,
 *   label[window, class] = (double)S / (double)W,  S = sum over the segments with start < s + W and end > s (0-based, half-open) of
 *   weight * (min(end, s + W) - max(start, s));  class 0 duplications (weight cp_num - 2), 1 copy-neutral / LOH (cp_num == 2, weight 1),
 *   2 deletions (weight 2 - cp_num).
 * Windows: win_start i64 [N], the DISTINCT starts, ascending within each chromosome's run; chrom_id i64 [n_chrom] ascending, the
 * chromosomes that have a window; chrom_off i64 [n_chrom + 1], a chromosome's first window, 0 first and N last.  Segments of all C
 * cohorts: seg_chrom (a chromosome id: one that chrom_id does not hold adds nothing), seg_start, seg_end i64 with 0 <= start < end <=
 * 2^40; seg_class u8 within [0, 2]; seg_weight i32 >= 1; seg_cohort i32 within [0, C).  The device entry point passes over a segment
 * outside these domains; the host twin refuses it, and a window table that is not as described.  Duplicate segments count twice.
 *   dig_cnv_segment_deltas: deltas i64 [C, 3, N + 1], zeroed by the call, of dig_cnv_segment_deltas_size(C, N) bytes: a difference
 *     array whose inclusive prefix sum along N is S.  One thread per segment, four binary searches into win_start: the windows a segment
 *     covers whole get + weight W at the first and - weight W one past the last, every window it covers in part its exact overlap v as
 *     + v at n and - v at n + 1.  64-bit integer atomics: the result does not depend on their order.
 *   dig_cnv_window_means: labels f64 [C, N, 3] from deltas, which it leaves as they are: the prefix sums in chunks of
 *     DIG_CNV_SCAN_CHUNK windows with a carry pass between.  carries: i64 scratch of dig_cnv_window_means_size(C, N) bytes.  S below
 *     2^53 is exact, and the division is IEEE: the bits of np.mean over the W positions.
 * 1 <= C < 2^20, 0 <= N < 2^31, 1 <= W < 2^31, 3 C (N + 1) < 2^40 (DIG_EINVAL otherwise; the size queries then return -1).  Buffers
 * at the alignment of their elements.  N = 0: nothing is written. */
#define DIG_CNV_SCAN_CHUNK 2048
int64_t dig_cnv_segment_deltas_size(int64_t C, int64_t N);
int64_t dig_cnv_window_means_size(int64_t C, int64_t N);
int dig_cnv_segment_deltas(const int64_t *win_start, const int64_t *chrom_id, const int64_t *chrom_off, int64_t n_chrom, int64_t N,
                           int64_t W, const int64_t *seg_chrom, const int64_t *seg_start, const int64_t *seg_end,
                           const uint8_t *seg_class, const int32_t *seg_weight, const int32_t *seg_cohort, int64_t n_seg, int64_t C,
                           int64_t *deltas, void *stream);
int dig_cnv_segment_deltas_host(const int64_t *win_start, const int64_t *chrom_id, const int64_t *chrom_off, int64_t n_chrom, int64_t N,
                                int64_t W, const int64_t *seg_chrom, const int64_t *seg_start, const int64_t *seg_end,
                                const uint8_t *seg_class, const int32_t *seg_weight, const int32_t *seg_cohort, int64_t n_seg,
                                int64_t C, int64_t *deltas, int device);
int dig_cnv_window_means(const int64_t *deltas, int64_t N, int64_t C, int64_t W, double *labels, int64_t *carries, void *stream);
int dig_cnv_window_means_host(const int64_t *deltas, int64_t N, int64_t C, int64_t W, double *labels, int device);

/* ---- the sequence model's substitution counts for many cohorts (additive: the ABI version stays) --------------- *
 * scripts/DigPretrain.py:179-208 sequenceModel: per cohort the K counts of (MUT_TYPE, CONTEXT) -- the rows of mk_mutation_context,
 * K = 192 or 3 072 -- over the rows that lie in a whitelisted window.  The (row, window) pairs come from dig_overlap_join_count/fill
 * with the windows as one-block elements and the rows of all C cohorts as mutations: mutation-major, so a row's pairs are
 * consecutive.  A row carries its table row (row_type i32, 0 .. K - 1; K = no table entry: counted nowhere) and its cohort
 * (row_cohort i32, 0 .. C - 1).
 *   dig_sequence_counts: counts i64 [C, K] = per cohort and type the rows with at least one pair -- a pair counts when its left
 *     neighbour belongs to another row.  Exact for one-base rows (END - START == 1), which restrict_mutations_by_bed(unique=True)
 *     keeps once however many windows hold them (mutation_tools.py:8-30).  1 <= K <= 3 072, C >= 1 (DIG_EINVAL otherwise).  A row or
 *     pair outside the tables is counted nowhere (the host twin refuses it).
 * counts is zeroed by the call; nothing is launched for n_pairs == 0.  A workgroup counts one cohort in 32-bit LDS counters and
 * adds each non-zero counter with one 64-bit integer atomic, so the result is order-independent. */
int dig_sequence_counts(const int32_t *pair_row, int64_t n_pairs, const int32_t *row_type, const int32_t *row_cohort, int64_t n,
                        int64_t K, int64_t C, int64_t *counts, void *stream);
int dig_sequence_counts_host(const int32_t *pair_row, int64_t n_pairs, const int32_t *row_type, const int32_t *row_cohort, int64_t n,
                             int64_t K, int64_t C, int64_t *counts, int device);

/* ---- the sites route's observed counts for many cohorts (additive: the ABI version stays) ----------------------- *
 * mutation_tools.py:233-281 tabulate_nonc_mutations_at_sites: a mutation row counts for a site row when CHROM, START, END, REF, ALT,
 * GENE, ANNOT, MUT_TYPE and CONTEXT all agree -- an exact match, not an overlap -- and per element OBS_SNV = matched (row, site) pairs,
 * OBS_SAMPLES = distinct samples among them.  The nine columns are three integers: pos = chrom << 40 | START, END, and attr, an
 * injective code of the six labels (formed by the caller from the sites file's own dictionaries; a negative row_attr matches nothing).
 * Sites: S rows sorted ascending by site_pos (the only column the search orders by), site_pos, site_end, site_attr i64 [S], site_elt
 * i32 [S] within [0, E).  Rows of all C cohorts, in any order: row_pos, row_end, row_attr i64 [n], row_sample i32 [n] = the GLOBAL
 * sample, row_cohort i32 [n]; sample_off i64 [C + 1] = a cohort's first global sample (0 first, n_samples last, as for
 * dig_gene_row_keys): a row's sample lies in its cohort's range.  S, E, C, n_samples < 2^31.
 *   dig_site_match_count: counts i32 [n] = the site rows with the row's pos, end and attr (one thread per row: a binary search for
 *     the first site at the position, then a walk over the equal-position run).
 *   The caller forms offsets i64 [n], the exclusive prefix sum of counts, and total, their sum (the two-call protocol of
 *     dig_overlap_join_count / fill).
 *   dig_site_match_keys: keys i64 [total]; match q of row i is keys[offsets[i] + q] = (cohort E + element) << sb | global sample, sb
 *     the bits of n_samples - 1 (DIG_EINVAL, from all three entry points, when the fields do not fit 63 bits).  keys is set to -1
 *     first and nothing is written outside [0, total): offsets that are not the prefix sum leave -1 keys, which count nowhere.
 *   The caller sorts the keys ascending (as for dig_gene_counts).
 *   dig_site_counts, from the sorted keys: obs_snv i32 [E, C] = keys per (element, cohort) -- a row that matches k site rows of an
 *     element counts k times, as the inner merge does -- and obs_samples i32 [E, C] = distinct keys per (element, cohort).
 * A row outside the tables (cohort outside [0, C), sample outside its cohort) and a site row with an element outside [0, E) match
 * nothing; the host twins refuse them, and a site table that is not ascending.  Every output is zeroed by its call; nothing is
 * launched for empty inputs; integer atomics, one per run of lanes with one destination, so order-independent. */
int dig_site_match_count(const int64_t *site_pos, const int64_t *site_end, const int64_t *site_attr, const int32_t *site_elt, int64_t S,
                         int64_t E, const int64_t *row_pos, const int64_t *row_end, const int64_t *row_attr, const int32_t *row_sample,
                         const int32_t *row_cohort, const int64_t *sample_off, int64_t n, int64_t C, int64_t n_samples, int32_t *counts,
                         void *stream);
int dig_site_match_count_host(const int64_t *site_pos, const int64_t *site_end, const int64_t *site_attr, const int32_t *site_elt,
                              int64_t S, int64_t E, const int64_t *row_pos, const int64_t *row_end, const int64_t *row_attr,
                              const int32_t *row_sample, const int32_t *row_cohort, const int64_t *sample_off, int64_t n, int64_t C,
                              int64_t n_samples, int32_t *counts, int device);
int dig_site_match_keys(const int64_t *site_pos, const int64_t *site_end, const int64_t *site_attr, const int32_t *site_elt, int64_t S,
                        int64_t E, const int64_t *row_pos, const int64_t *row_end, const int64_t *row_attr, const int32_t *row_sample,
                        const int32_t *row_cohort, const int64_t *sample_off, int64_t n, int64_t C, int64_t n_samples,
                        const int64_t *offsets, int64_t total, int64_t *keys, void *stream);
int dig_site_match_keys_host(const int64_t *site_pos, const int64_t *site_end, const int64_t *site_attr, const int32_t *site_elt,
                             int64_t S, int64_t E, const int64_t *row_pos, const int64_t *row_end, const int64_t *row_attr,
                             const int32_t *row_sample, const int32_t *row_cohort, const int64_t *sample_off, int64_t n, int64_t C,
                             int64_t n_samples, const int64_t *offsets, int64_t total, int64_t *keys, int device);
int dig_site_counts(const int64_t *keys_sorted, int64_t total, int64_t E, int64_t C, int64_t n_samples, int32_t *obs_snv,
                    int32_t *obs_samples, void *stream);
int dig_site_counts_host(const int64_t *keys_sorted, int64_t total, int64_t E, int64_t C, int64_t n_samples, int32_t *obs_snv,
                         int32_t *obs_samples, int device);

/* ---- the hits of the per-base route for many cohorts (additive: the ABI version stays) -------------------------- *
 * The entries of a score plane that pass a per-cohort cut, in the row order of the reference's nb_model frame (nb_model.py:188-234:
 * one block per region, tiles ascending; one frame per cohort), without the frame being built.  score f64 [C, R, T] (the p-values
 * of dig_tiled_nb_test), n_valid i32 [R] as dig_base_tile_probs* writes it (<= 0, the -1 of an unevaluated region included: the
 * row has no tiles), cut f64 [C].  Tile (c, r, t) is a HIT when t < n_valid[r] and score[c, r, t] <= cut[c]: a NaN score or a NaN
 * cut never hits, cut = +inf takes every existing tile with a non-NaN score.  C R < 2^31 and T < 2^31 (DIG_EINVAL otherwise,
 * before anything is read).  Every typed pointer needs the alignment of its element and no more.
 *   dig_tile_select_count: counts i32 [C R] = the hits of row (c, r), zeroed and written by the call (one streaming pass over the
 *     plane; one integer atomic per run of lanes with one row and a hit).
 *   The caller forms offsets i64 [C R], the exclusive prefix sum of counts, and total, their sum (the two-call protocol of
 *     dig_overlap_join_count / fill).
 *   dig_tile_select_fill: hit h of row (c, r), tiles ascending, goes to slot offsets[c R + r] + h -- hits lie cohort-major, then by
 *     region, then by tile -- as hit_region i32, hit_tile i32, hit_score f64 and, from the planes pt, exp_in f64 and k i32
 *     [C, R, T], hit_pt, hit_exp, hit_k [total].  Each output and each plane may be NULL: an output that is NULL, or whose plane
 *     is, is skipped.  A row writes only inside its own slots [offsets[row], offsets[row + 1]) (total behind the last row) and
 *     inside [0, total): offsets that are not the prefix sum write nowhere else (the host twin refuses them).
 * Integer atomics only, so order-independent; nothing is launched for empty inputs. */
int dig_tile_select_count(const double *score, const int32_t *n_valid, const double *cut, int64_t C, int64_t R, int64_t T,
                          int32_t *counts, void *stream);
int dig_tile_select_count_host(const double *score, const int32_t *n_valid, const double *cut, int64_t C, int64_t R, int64_t T,
                               int32_t *counts, int device);
int dig_tile_select_fill(const double *score, const int32_t *n_valid, const double *cut, int64_t C, int64_t R, int64_t T,
                         const int64_t *offsets, int64_t total, const double *pt, const double *exp_in, const int32_t *k,
                         int32_t *hit_region, int32_t *hit_tile, double *hit_score, double *hit_pt, double *hit_exp, int32_t *hit_k,
                         void *stream);
int dig_tile_select_fill_host(const double *score, const int32_t *n_valid, const double *cut, int64_t C, int64_t R, int64_t T,
                              const int64_t *offsets, int64_t total, const double *pt, const double *exp_in, const int32_t *k,
                              int32_t *hit_region, int32_t *hit_tile, double *hit_score, double *hit_pt, double *hit_exp,
                              int32_t *hit_k, int device);

/* ---- the calls of the element route: ragged lists out of a score plane and back (additive: the ABI version stays) -- *
 * score f64 [rows, n] (a row: one p-value column of one cohort over n elements), cut f64 [rows].  Element (r, e) is SELECTED when
 * score[r, e] <= cut[r]: the rule of dig_tile_select_* without n_valid.  A NaN score or a NaN cut selects nothing, cut = +inf takes
 * every score that is a number.  A row is cut into chunks of K = dig_row_select_chunk() consecutive elements, chunks =
 * ceil(n / K) per row, chunk w = r * chunks + c; one wave owns a chunk.  rows, n >= 0, n < 2^31, rows * chunks < 2^31 and
 * total >= 0 (DIG_EINVAL otherwise, before anything is read).  Every typed pointer needs the alignment of its element and no more.
 *   dig_row_select_counts_size(rows, n) = rows * chunks, the elements of counts and of offsets (-1 for sizes that are refused).
 *   dig_row_select_count: counts i32 [rows * chunks] = the selected elements of every chunk; each slot is written once, by the
 *     chunk's wave: no atomics, and counts need not be zeroed.
 *   The caller forms offsets i64 [rows * chunks], the exclusive prefix sum of counts, and total, their sum.
 *   dig_row_select_fill: the selected elements in row-major order, ascending in e within a row, as hit_index i32 [total] (e) and
 *     hit_score f64 [total]; each may be NULL.  A chunk writes only inside its own slots [offsets[w], offsets[w + 1]) (total behind
 *     the last chunk) and inside [0, total): offsets that are not the prefix sum write nowhere else (the host twin refuses them).
 *   dig_row_scatter: the inverse of the fill.  out f64 [rows, n]: out[r, e] = values[slot of (r, e)] where (r, e) is selected and
 *     its slot lies in the chunk's range, `fill` elsewhere; values f64 [total].  Every element of out is written.
 * No atomics; nothing is launched for empty inputs. */
int64_t dig_row_select_chunk(void);
int64_t dig_row_select_counts_size(int64_t rows, int64_t n);
int dig_row_select_count(const double *score, const double *cut, int64_t rows, int64_t n, int32_t *counts, void *stream);
int dig_row_select_count_host(const double *score, const double *cut, int64_t rows, int64_t n, int32_t *counts, int device);
int dig_row_select_fill(const double *score, const double *cut, int64_t rows, int64_t n, const int64_t *offsets, int64_t total,
                        int32_t *hit_index, double *hit_score, void *stream);
int dig_row_select_fill_host(const double *score, const double *cut, int64_t rows, int64_t n, const int64_t *offsets, int64_t total,
                             int32_t *hit_index, double *hit_score, int device);
int dig_row_scatter(const double *score, const double *cut, int64_t rows, int64_t n, const int64_t *offsets, int64_t total,
                    const double *values, double fill, double *out, void *stream);
int dig_row_scatter_host(const double *score, const double *cut, int64_t rows, int64_t n, const int64_t *offsets, int64_t total,
                         const double *values, double fill, double *out, int device);

/* ---- the meta-cohorts of the element route: groups of cohorts combined per element (additive: the ABI version stays) -- *
 * Planes are f64 [R, C, E] (R stacked columns, C cohorts, E elements, E contiguous); member u8 [M, C]: non-zero where cohort c
 * belongs to group g (a cohort may be in many groups, or in none); outputs are [R, M, E].  R, C, E, M >= 0, C <= 64, M <= 32 per
 * call, E < 2^31 and R * ceil(E / 128) < 2^31 (DIG_EINVAL otherwise, before anything is read).  Every typed pointer needs the
 * alignment of its element and no more (16-byte loads and stores are used where an address allows them).
 *   dig_group_fisher: Fisher's method over the TESTABLE members of a group, chi2.sf(-2 sum ln p_c, 2 m).  A member whose p is NaN
 *     is not testable: it adds nothing and is not counted.  With s = the sum of -ln p over the testable members in ascending c and
 *     m their number, out_n i32 [R, M, E] = m (out_n may be NULL) and out_p =
 *       m = 0 (an empty group included)   NaN
 *       m = 1                             that member's p, bit for bit
 *       m = 2                             what dig_fisher gives for the pair (p_a, p_b), a < b, bit for bit
 *       m >= 3                            Q(m, s) = e^-s sum_{j<m} s^j / j! as exp(log(r) - s), r = 1 + s/1 (1 + s/2 (... (1 + s/(m-1))))
 *                                         by Horner; s < 0 (a p above 1) -> 1.0, s = +inf (a p of 0) -> 0.0, a NaN s -> NaN
 *   dig_group_sums: out[r, g, e] = the sum of x[r, c, e] over the members c of g in ascending c, one IEEE addition each, from +0.0;
 *     with a gate f64 [R, C, E] (NULL: none) only over the members whose gate[r, c, e] is not NaN.  Nothing to add: 0.0.
 * Every p (x, gate) is read once per call and every output written once, by its owner: no atomics, outputs need not be zeroed.
 * Nothing is launched when R M E = 0. */
int dig_group_fisher(const double *p, const uint8_t *member, int64_t R, int64_t C, int64_t E, int64_t M, double *out_p, int32_t *out_n,
                     void *stream);
int dig_group_fisher_host(const double *p, const uint8_t *member, int64_t R, int64_t C, int64_t E, int64_t M, double *out_p,
                          int32_t *out_n, int device);
int dig_group_sums(const double *x, const double *gate, const uint8_t *member, int64_t R, int64_t C, int64_t E, int64_t M, double *out,
                   void *stream);
int dig_group_sums_host(const double *x, const double *gate, const uint8_t *member, int64_t R, int64_t C, int64_t E, int64_t M,
                        double *out, int device);

/* ---- the power of the element route's burden test: critical counts and the chance of reaching them (additive: the ABI version
 * stays) ---------------------------------------------------------------------------------------------------------------------- *
 * Planes alpha, theta, pi are f64 [rows, n] (rows = cohorts, n elements, n contiguous); scale f64 [rows] (NULL: 1), level f64
 * [rows]; folds f64 [n_folds], in device memory for dig_nb_power.  Per pair (r, e), every product ONE IEEE multiplication, left to
 * right, without contraction:
 *   theta' = theta[r, e] * scale[r];   p(f) = 1 / ((theta' * pi[r, e]) * f + 1)      (f = 1: the p of the statistics block)
 *   k_crit[r, e] = K = the smallest integer k in [0, k_max] with nb_pvalue_greater_midp(k, alpha, p(1)) <= level[r]
 *     (nb_model.py:271-278, the statistic of dig_nb_midp_upper; it falls strictly in k, M(k) - M(k + 1) = (pmf(k) + pmf(k + 1)) / 2,
 *     so K is well defined).  K = -1 where (a) no k <= k_max reaches the level, (b) the statistic is NaN (alpha or p outside what
 *     dig_nb_midp_upper accepts, a NaN input), (c) level[r] is not inside (0, 1) (a NaN level included).
 *   power[j, r, e] = nb_pvalue_greater(K, alpha, p(folds[j])) (nb_model.py:243-256, what dig_nb_greater gives: P(X >= K) under the
 *     reference's alternative of a fold f of selection, transfer_tools.py:1290-1291, with its k == 0 -> 1 clause and its pmf
 *     fallback); 0.0 where K = -1 by (a), NaN where K = -1 by (b) or (c).
 * k_crit i32 [rows, n], power f64 [n_folds, rows, n]; each is written once by its owner: no atomics, no workspace, outputs need not
 * be zeroed.  The statistic is the project's own (1e-6 relative down to 1e-250, README): where neither M(K - 1) nor M(K) lies within
 * that of the level, K is the reference's count exactly.
 * DIG_EINVAL, before anything is read or launched: negative rows or n; n_folds outside [0, DIG_NB_POWER_MAX_FOLDS]; k_max outside
 * [0, 2^30]; n_folds > 0 with folds NULL; power NULL with n_folds > 0 or non-NULL with n_folds = 0; n >= 2^31 or rows *
 * ceil(n / 256) >= 2^31 (a chunk per workgroup); with rows * n > 0 a NULL alpha, theta, pi, level or k_crit.  The host twin also
 * refuses a fold that is not finite and > 0 (the device form cannot look: such a fold gives what the formulas give).  Nothing is
 * launched when rows * n = 0. */
#define DIG_NB_POWER_MAX_FOLDS 8
int dig_nb_power(const double *alpha, const double *theta, const double *pi, const double *scale, const double *level, int64_t rows,
                 int64_t n, const double *folds, int n_folds, int32_t k_max, int32_t *k_crit, double *power, void *stream);
int dig_nb_power_host(const double *alpha, const double *theta, const double *pi, const double *scale, const double *level,
                      int64_t rows, int64_t n, const double *folds, int n_folds, int32_t k_max, int32_t *k_crit, double *power,
                      int device);

/* ---- pairs of the element route: co-occurrence and exclusivity of called elements across a cohort's samples (additive: the ABI
 * version stays) ----------------------------------------------------------------------------------------------------------------- *
 * The rule, for one cohort of n samples and H entering elements h = 0 .. H - 1 (nothing in the reference does this; it is pinned to
 * exact integer arithmetic and to scipy):
 *   row h    the set of samples with at least one kept mutation in element h, as n bits of W u64 words: sample s is bit s % 64 of word
 *            s / 64; the bits behind sample n - 1 are zero.
 *   counts   for every pair i < j: r = |row i|, k = |row j|, a = |row i AND row j| (N_BOTH), lo = max(0, r + k - n), hi = min(r, k).
 *   density  pmf(x) = C(k, x) C(n - k, r - x) / C(n, r).
 *   PVAL_COOCCUR  = sum_{x = a .. hi} pmf(x)   (scipy hypergeom.sf(a - 1, n, k, r); fisher_exact(alternative='greater'))
 *   PVAL_EXCLUSIVE = sum_{x = lo .. a} pmf(x)  (hypergeom.cdf(a, n, k, r); alternative='less')
 *            A pair with r = 0, k = 0, r = n or k = n has both equal to 1.
 *   order    pairs are listed per cohort in row-major upper-triangle order, idx(i, j) = i (2 H - i - 1) / 2 + (j - i - 1);
 *            pair_ptr[c] is the sum of H_c (H_c - 1) / 2 over the earlier cohorts.
 *   tails    pmf(a) = exp of a sum of table entries ln(x!) (lnfact, x = 0 .. n_max, lgamma(x + 1), filled once per call).  With
 *            mode = floor((r + 1)(k + 1) / (n + 2)): for a >= mode the upper tail, otherwise the lower one, is summed outward from
 *            a by the ratio recurrence pmf(x + 1) / pmf(x) = (k - x)(r - x) / ((x + 1)(n - k - r + x + 1)); its terms fall, and it
 *            stops when a term is no more than 2^-56 of the sum or the support ends.  The other tail is 1 - that + pmf(a).  Both are
 *            capped at 1.  The small tail is a sum of positive terms, the large one is at least about a half.
 *   limits   n <= DIG_PAIR_MAX_SAMPLES = 65 536, H <= DIG_PAIR_MAX_ROWS = 8 192 per cohort, fewer than 2^31 pairs per call.
 *
 * dig_pair_bits: (row, sample) keys -> the stacked bit matrix bits u64 [H_total, W], which the entry point zeroes first.  row i32
 * [n_keys]: a row of the matrix, -1 (any value outside [0, H_total)) where the key's element does not enter; sample i32 [n_keys]:
 * the cohort-local sample index (a value outside [0, 64 W) sets nothing).  One thread per key and one 32-bit atomic OR; a repeated
 * key is harmless.  W: the call's words per row, even (16-byte rows), 2 <= W <= 1024.
 * DIG_EINVAL before anything is launched: negative n_keys or H_total; W odd or outside [2, 1024]; H_total >= 2^31; n_keys >= 2^39;
 * with H_total > 0 a NULL bits or one that is not 16-byte aligned; with n_keys > 0 a NULL row or sample.
 *
 * dig_pair_fisher: bits -> per row its popcount n_row i32 [H_total], per pair n_both i32, pval_cooccur f64 and pval_exclusive f64 at
 * the pair's slot pair_ptr[c] + idx(i, j) ([n_pairs]); lnfact f64 [n_max + 1] is the table, an output the caller provides room for
 * (the only workspace).  row_ptr i64 [C + 1] (cohort c owns the rows row_ptr[c] .. row_ptr[c + 1] - 1), n_samples i32 [C], pair_ptr
 * i64 [C + 1]; tiles i32 [n_tiles, 3] = (cohort, block i, block j), one per DIG_PAIR_TILE x DIG_PAIR_TILE = 64 x 64 tile of a
 * cohort's pair matrix with block i <= block j and 64 block j < H_c, in any order (engine.pair_tiles builds it: a few KB); a
 * workgroup per tile, a diagonal tile does its upper triangle.  n_max >= every n_samples[c] and h_max >= every H_c are what the
 * caller declares of the device arrays: the limits are checked on them, the table is sized by n_max, and the kernel clips a cohort
 * to them and writes no slot outside [0, n_pairs).  A pair whose counts cannot belong to n samples (a bit set behind sample
 * n - 1) gets NaN p-values.  The panels go through LDS DIG_PAIR_CHUNK_BITS = 2 048 samples at a time.
 * dig_pair_counts: the same without the tail rule and the table: n_row and n_both only.
 * DIG_EINVAL before anything is launched: a negative size; n_max > 65 536; h_max > 8 192; n_pairs >= 2^31; n_tiles, C or H_total >=
 * 2^31; W odd, outside [2, 1024] or below n_max / 64; with H_total > 0 a NULL bits or one that is not 16-byte aligned, or a NULL
 * n_row; a NULL lnfact; with n_pairs > 0 a NULL n_both, pval_cooccur or pval_exclusive; with n_tiles > 0 a NULL row_ptr, n_samples,
 * pair_ptr or tiles.  The host twins also check the plan arrays themselves: row_ptr from 0 to H_total with 0 <= H_c <= h_max,
 * 0 <= n_samples[c] <= n_max, pair_ptr[c + 1] - pair_ptr[c] = H_c (H_c - 1) / 2 up to n_pairs, every tile inside its cohort.  Device
 * form and twin run the same kernels: their outputs are equal bit for bit. */
#define DIG_PAIR_MAX_SAMPLES 65536
#define DIG_PAIR_MAX_ROWS 8192
#define DIG_PAIR_TILE 64
#define DIG_PAIR_CHUNK_BITS 2048
int dig_pair_bits(const int32_t *row, const int32_t *sample, int64_t n_keys, int64_t H_total, int64_t W, uint64_t *bits, void *stream);
int dig_pair_bits_host(const int32_t *row, const int32_t *sample, int64_t n_keys, int64_t H_total, int64_t W, uint64_t *bits,
                       int device);
int dig_pair_fisher(const uint64_t *bits, int64_t H_total, int64_t W, const int64_t *row_ptr, const int32_t *n_samples,
                    const int64_t *pair_ptr, int64_t C, const int32_t *tiles, int64_t n_tiles, int64_t n_pairs, int32_t n_max,
                    int32_t h_max, double *lnfact, int32_t *n_row, int32_t *n_both, double *pval_cooccur, double *pval_exclusive,
                    void *stream);
int dig_pair_fisher_host(const uint64_t *bits, int64_t H_total, int64_t W, const int64_t *row_ptr, const int32_t *n_samples,
                         const int64_t *pair_ptr, int64_t C, const int32_t *tiles, int64_t n_tiles, int64_t n_pairs, int32_t n_max,
                         int32_t h_max, double *lnfact, int32_t *n_row, int32_t *n_both, double *pval_cooccur,
                         double *pval_exclusive, int device);
int dig_pair_counts(const uint64_t *bits, int64_t H_total, int64_t W, const int64_t *row_ptr, const int32_t *n_samples,
                    const int64_t *pair_ptr, int64_t C, const int32_t *tiles, int64_t n_tiles, int64_t n_pairs, int32_t n_max,
                    int32_t h_max, int32_t *n_row, int32_t *n_both, void *stream);
int dig_pair_counts_host(const uint64_t *bits, int64_t H_total, int64_t W, const int64_t *row_ptr, const int32_t *n_samples,
                         const int64_t *pair_ptr, int64_t C, const int32_t *tiles, int64_t n_tiles, int64_t n_pairs, int32_t n_max,
                         int32_t h_max, int32_t *n_row, int32_t *n_both, int device);

/* ---- the map report: a map's bins merged into larger windows, the region test per window, the scores of a cohort (additive: the
 * ABI version stays) ------------------------------------------------------------------------------------------------------------- *
 * Reference: gp_tools.merge_windows (sequence_model/gp_tools.py:125-160) and calibration_score_by_pvals (:117-121).
 * Inputs: C maps on one (CHROM, START)-sorted grid of N bins, cohort-major: mu_cm (Y_PRED), std_cm (STD) f64 [C, N], y_cm (Y_TRUE) i32
 * [C, N], flag_cm (FLAG) u8 [C, N] (may be NULL with drop_flagged = 0, when it is not read).  Merged windows: with W the grid's window
 * and s >= 1 the scale, the key of bin i is (chrom[i], start[i] / (s W)); the M merged windows are the runs of equal key in grid
 * order, run_ptr i64 [M + 1] (window m = bins run_ptr[m] .. run_ptr[m + 1] - 1; the caller builds it once per scale; device memory
 * for dig_map_windows).  Bins missing from the grid add nothing; a window without a bin does not exist.
 *   dig_map_windows, per cohort c and window m, with the gate g = 1, and g = 0 for a bin with flag != 0 when drop_flagged = 1:
 *     n_bins i32 = sum g;   y_true i64 = sum g y;   y_pred f64 = sum g mu;   std f64 = sqrt(sum g std^2)
 *     -- the two float sums are SEQUENTIAL IEEE double additions in ascending bin order from +0.0 (a gated-out bin adds +0.0), std * std
 *     rounded before it is added (no fused multiply-add), the square root correctly rounded: np.cumsum over the run gives the same bits.
 *     pval f64: NaN for n_bins = 0; otherwise (alpha, theta) = normal_params_to_gamma(y_pred, std), p = 1 / (theta + 1) and
 *       tail = 0: nb_pvalue_greater_midp(y_true, alpha, p) (nb_model.py:271-278, what dig_nb_midp_upper gives: the burden test);
 *       tail = 1: nb_pvalue_midp(y_true, alpha, p) (nb_model.py:316-337, what dig_nb_midp_twosided gives);
 *     NaN where the reference's expression is NaN (y_pred <= 0, std = 0, a NaN input).
 *     The five outputs are cohort-major [C, M] (M contiguous), each element written once by its owner: no atomics, no workspace, one
 *     launch.
 *   dig_map_scores, per cohort over the windows with n_bins > 0:
 *     counts i64 [C, 7]: N_WINDOWS; N_TESTED (pval not NaN); OBS_TOTAL = sum y_true; N_BELOW[a] = the windows with pval < a, strict,
 *       for a = 0.05, 0.01, 0.001, 0.0001;
 *     sums f64 [C, 4]: EXP_TOTAL = sum y_pred; and, with mx = (double)OBS_TOTAL / (double)N_WINDOWS, my = EXP_TOTAL / (double)N_WINDOWS,
 *       dx = (double)y_true - mx, dy = y_pred - my:  Sxx = sum dx dx, Syy = sum dy dy, Sxy = sum dx dy (every product rounded before it
 *       is added).  The caller forms R2 = Sxy^2 / (Sxx Syy), the fractions and the calibration score.
 *     The order of the four float sums is fixed by (M, C) alone: the windows of a cohort in chunks of 1024 (the last one shorter); in a
 *     chunk, lane t of 256 adds the terms of windows t, t + 256, t + 512, t + 768 in that order from +0.0 (a window with n_bins = 0 or
 *     past M adds +0.0), the lane sums are folded by halves (t += t + 128, then + 64, ... + 1), and the chunk sums are added first to last
 *     from +0.0.  Any stream, any run, and the host twins: the same bits.
 *     workspace: at least dig_map_scores_workspace(C, M) bytes, 8-byte aligned; it need not be zeroed.  C > 0 with M = 0: all zero.
 * DIG_EINVAL, before anything is read or launched: negative C, N or M; tail or drop_flagged outside {0, 1}; drop_flagged with a NULL
 * flag_cm (and C N > 0); C >= 2^31, N or M >= 2^40; C * window groups >= 2^31 (dig_map_windows: a group is 4096 / (N / M), at least 1
 * and at most 256, neighbouring windows) or C * ceil(M / 1024) >= 2^31 (dig_map_scores); with C M > 0 a NULL run_ptr or output, with
 * N > 0 too a NULL mu_cm, std_cm or y_cm; for dig_map_scores with C > 0 a NULL counts or sums, with M > 0 a NULL plane or workspace, a
 * workspace that is too small or not 8-byte aligned.  dig_map_windows_host also refuses a run_ptr that begins below 0, does not end at
 * N or decreases anywhere (the device form cannot look: it clamps every value into [its left neighbour, N], so a bad run_ptr reads
 * nothing outside the tables).  Nothing is launched when C M = 0 (dig_map_windows) or C = 0 (dig_map_scores). */
int dig_map_windows(const double *mu_cm, const double *std_cm, const int32_t *y_cm, const uint8_t *flag_cm, int64_t C, int64_t N,
                    const int64_t *run_ptr, int64_t M, int drop_flagged, int tail, int32_t *n_bins, int64_t *y_true, double *y_pred,
                    double *std, double *pval, void *stream);
int dig_map_windows_host(const double *mu_cm, const double *std_cm, const int32_t *y_cm, const uint8_t *flag_cm, int64_t C, int64_t N,
                         const int64_t *run_ptr, int64_t M, int drop_flagged, int tail, int32_t *n_bins, int64_t *y_true,
                         double *y_pred, double *std, double *pval, int device);
int64_t dig_map_scores_workspace(int64_t C, int64_t M);
int dig_map_scores(const int32_t *n_bins, const int64_t *y_true, const double *y_pred, const double *pval, int64_t C, int64_t M,
                   int64_t *counts, double *sums, void *workspace, int64_t workspace_bytes, void *stream);
int dig_map_scores_host(const int32_t *n_bins, const int64_t *y_true, const double *y_pred, const double *pval, int64_t C, int64_t M,
                        int64_t *counts, double *sums, int device);

/* ---- the per-base route's counts by sample for many cohorts (additive: the ABI version stays) ------------------- *
 * dig_tile_mut_counts counts rows, whoever they belong to.  These two entry points count them per sample: with n(c, r, t, s) the
 * rows of GLOBAL sample s that dig_tile_mut_counts would count in tile (c, r, t) -- the same pairs, the same skip rules --
 *   k_cap[c, r, t]     = sum over the kept samples of min(n, cap)     (cap <= 0: no cap)
 *   k_samples[c, r, t] = the kept samples with n > 0
 * i32 [C, R, n_tiles] each.  mut_sample i32 [n_mut]: the row's global sample (the samples of all cohorts numbered as one list of
 * n_samples; equal labels in two cohorts are two samples); keep u8 [n_samples] or NULL: a sample with keep == 0 counts nowhere.
 *   dig_tile_sample_keys: keys i64 [n_pairs], one per (mutation, region) pair of dig_overlap_join_count/fill:
 *     (((cohort R + region) n_tiles + tile) << sb) | global sample, sb = the bits that hold the values 0 .. n_samples; a pair that
 *     counts nowhere (START in front of the region, tile at or past n_valid[region] or n_tiles, cohort outside [0, C), sample outside
 *     [0, n_samples) or not kept, pair outside the tables) gets the all-ones 63-bit key INT64_MAX, which sorts behind every real one.
 *   The caller sorts the keys ascending.
 *   dig_tile_sample_counts: a run of equal keys is one (tile, sample) with n = its length; both planes are zeroed by the call, either
 *     may be NULL and is then skipped.  Negative keys, the all-ones key and keys of a tile outside the planes are passed over.
 *     n < 2^31.  One integer atomic per plane, wave segment and tile: the cost does not depend on how many rows a sample has in a
 *     tile.  Integer atomics only, so order-independent.
 * DIG_EINVAL, before anything is read or launched, when C, R, n_tiles or n_samples reach 2^31 or the key's fields do not fit 63
 * bits.  Every typed pointer needs the alignment of its element and no more.  The host twins refuse pairs outside the tables, a row
 * of a cohort within [0, C) whose sample is outside [0, n_samples), and keys that are not ascending. */
int dig_tile_sample_keys(const int32_t *pair_mut, const int32_t *pair_reg, int64_t n_pairs, const int64_t *mut_start, int64_t n_mut,
                         const int32_t *mut_cohort, const int32_t *mut_sample, const uint8_t *keep, const int64_t *first_pos,
                         const int32_t *n_valid, int binsize, int64_t n_tiles, int64_t R, int64_t C, int64_t n_samples,
                         int64_t *keys, void *stream);
int dig_tile_sample_keys_host(const int32_t *pair_mut, const int32_t *pair_reg, int64_t n_pairs, const int64_t *mut_start,
                              int64_t n_mut, const int32_t *mut_cohort, const int32_t *mut_sample, const uint8_t *keep,
                              const int64_t *first_pos, const int32_t *n_valid, int binsize, int64_t n_tiles, int64_t R, int64_t C,
                              int64_t n_samples, int64_t *keys, int device);
int dig_tile_sample_counts(const int64_t *keys_sorted, int64_t n, int64_t C, int64_t R, int64_t n_tiles, int64_t n_samples,
                           int64_t cap, int32_t *k_cap, int32_t *k_samples, void *stream);
int dig_tile_sample_counts_host(const int64_t *keys_sorted, int64_t n, int64_t C, int64_t R, int64_t n_tiles, int64_t n_samples,
                                int64_t cap, int32_t *k_cap, int32_t *k_samples, int device);

/* ---- the per-base route for the mutated tiles only (additive: the ABI version stays) ------------------------------ *
 * The dense route keeps four [C, R, n_tiles] planes.  These entry points keep nothing of that size: a census of the regions
 * ([R] and [C, R] arrays), one key per (mutation, region) pair, and one test per run of equal keys -- a tile that holds a row.
 * Genome, chromosome and region arguments, s_prob [C, 4^(2 n_up + 1)], n_up, binsize and n_tiles as dig_base_tile_probs_ctx
 * takes them; both genome walkers clamp every word index into [0, n_words).
 *   dig_tile_census_workspace(C, n_up): the bytes of dig_tile_census's workspace, ceil(C / 64) (at least 1) words of 8 bytes per
 *     context; 0 for arguments outside their domains.  The workspace is aligned to 8 bytes.
 *   dig_tile_census: first_pos i64 [R], n_valid i32 [R]: bit-equal to what dig_base_tile_probs_ctx writes.
 *     denom f64 [C, R]: the region's sum of s_prob over its positions (a window that holds a letter other than ACGT adds nothing),
 *     what the dense route divides by, regrouped by context: exact integer context counts times the table, added in one order -- lane l
 *     of a 64-lane wave takes the contexts l, l + 64, ... ascending (fma), then the lanes fold by halves (32, 16, ..., 1).  No
 *     floating-point atomics: the bits depend on the region and the table alone.
 *     n_positive i32 [C, R]: the tiles t < n_valid[r] that hold at least one all-ACGT window with s_prob[c][context] > 0 -- the
 *     tiles whose dense pt is > 0.  Cohorts go in passes of 64 (one mask word per context).
 *     A region whose chromosome id is outside [0, n_chrom) is read as one without positions.  R < 2^31 (a workgroup per region).
 *   dig_sparse_tile_keys: keys i64 [n_pairs], one per (mutation, region) pair of dig_overlap_join_count/fill, under the skip rules of
 *     dig_tile_mut_counts: (cohort R + region) n_tiles + tile for the tile that holds the row's START; INT64_MAX for a pair that counts
 *     nowhere (START in front of the region, tile at or past n_valid[region] or n_tiles, cohort outside [0, C), pair outside the tables).
 *   The caller sorts the keys ascending.
 *   dig_sparse_tile_test: a run of equal keys is one mutated tile with k = its length.  At the index of the run's FIRST key:
 *     out_cohort, out_region, out_tile, out_k i32 and out_pt (the sum of s_prob[c] over the tile's positions in position order,
 *     divided by denom[c, r]), out_exp (pt mu), out_pval f64 -- the arithmetic of dig_tiled_nb_test through the same device functions.
 *     Every other index gets cohort = region = tile = -1, k = 0 and NaN: all n entries of all seven outputs are written.  A key
 *     outside [0, C R n_tiles) (negative, INT64_MAX) is passed over and never dereferenced.  denom, mu, sigma f64 [C, R].  n < 2^31.
 *     One search per run: the cost does not depend on how many rows a tile holds.
 * DIG_EINVAL, before anything is read or launched, when C, R or n_tiles reach 2^31 or C R n_tiles does not fit 62 bits.  Every typed
 * pointer needs the alignment of its element and no more.  The host twins refuse regions outside the genome table (and what
 * dig_base_tile_probs_ctx_host refuses of a region), pairs outside the tables and keys that are not ascending. */
int64_t dig_tile_census_workspace(int64_t C, int n_up);
int dig_tile_census(const uint32_t *genome_words, int64_t n_words, const int64_t *chrom_off, const int64_t *chrom_len, int n_chrom,
                    const int32_t *reg_chrom, const int64_t *reg_start, const int64_t *reg_end, int64_t R, const double *s_prob,
                    int64_t C, int n_up, int binsize, int64_t n_tiles, int64_t *first_pos, int32_t *n_valid, double *denom,
                    int32_t *n_positive, void *workspace, int64_t workspace_bytes, void *stream);
int dig_tile_census_host(const uint32_t *genome_words, int64_t n_words, const int64_t *chrom_off, const int64_t *chrom_len,
                         int n_chrom, const int32_t *reg_chrom, const int64_t *reg_start, const int64_t *reg_end, int64_t R,
                         const double *s_prob, int64_t C, int n_up, int binsize, int64_t n_tiles, int64_t *first_pos,
                         int32_t *n_valid, double *denom, int32_t *n_positive, int device);
int dig_sparse_tile_keys(const int32_t *pair_mut, const int32_t *pair_reg, int64_t n_pairs, const int64_t *mut_start, int64_t n_mut,
                         const int32_t *mut_cohort, const int64_t *first_pos, const int32_t *n_valid, int binsize, int64_t n_tiles,
                         int64_t R, int64_t C, int64_t *keys, void *stream);
int dig_sparse_tile_keys_host(const int32_t *pair_mut, const int32_t *pair_reg, int64_t n_pairs, const int64_t *mut_start,
                              int64_t n_mut, const int32_t *mut_cohort, const int64_t *first_pos, const int32_t *n_valid,
                              int binsize, int64_t n_tiles, int64_t R, int64_t C, int64_t *keys, int device);
int dig_sparse_tile_test(const uint32_t *genome_words, int64_t n_words, const int64_t *chrom_off, const int64_t *chrom_len,
                         int n_chrom, const int32_t *reg_chrom, const int64_t *reg_start, const int64_t *reg_end, int64_t R,
                         const double *s_prob, int64_t C, int n_up, int binsize, int64_t n_tiles, const double *denom,
                         const double *mu, const double *sigma, const int64_t *keys_sorted, int64_t n, int32_t *out_cohort,
                         int32_t *out_region, int32_t *out_tile, int32_t *out_k, double *out_pt, double *out_exp, double *out_pval,
                         void *stream);
int dig_sparse_tile_test_host(const uint32_t *genome_words, int64_t n_words, const int64_t *chrom_off, const int64_t *chrom_len,
                              int n_chrom, const int32_t *reg_chrom, const int64_t *reg_start, const int64_t *reg_end, int64_t R,
                              const double *s_prob, int64_t C, int n_up, int binsize, int64_t n_tiles, const double *denom,
                              const double *mu, const double *sigma, const int64_t *keys_sorted, int64_t n, int32_t *out_cohort,
                              int32_t *out_region, int32_t *out_tile, int32_t *out_k, double *out_pt, double *out_exp,
                              double *out_pval, int device);

/* ---- sliding windows in the per-base route (additive: the ABI version stays) --------------------------------------- *
 * The NB test of every run of `width` = m consecutive tiles of a region, from the base planes pt f64, k i32 [C, R, T] and n_valid
 * i32 [R] as dig_base_tile_probs* and dig_tile_mut_counts (or dig_tile_sample_counts) leave them; mu, sigma f64 [C, R].  With
 * nv = min(n_valid[r], T) (n_valid[r] <= 0: the region has no tiles):
 *   n_windows i32 [R]: 0 when nv <= 0, else max(nv - m + 1, 1).  Window t of region r covers the tiles t .. min(t + m, nv) - 1: a
 *     region has full windows only, or a single window over all its tiles when it has fewer than m.
 *   pt_w f64 [C, R, T]: the window's pt values added LEFT TO RIGHT in float64, ((pt[t] + pt[t + 1]) + pt[t + 2]) + ..., the first
 *     term taken as it is.  The order is part of the contract.   k_w i32 [C, R, T]: the integer sum.
 *   pval_w, exp_w f64 [C, R, T]: alpha, theta from (mu, sigma), p = 1 / (pt_w theta + 1), pval_w = nb_exact(k_w, alpha, p),
 *     exp_w = pt_w mu -- the device functions of dig_tiled_nb_test: equal inputs give equal bits, and width 1 gives its planes.
 *   For t >= n_windows[r]: pt_w is the NaN of the base planes, k_w 0, and exp_w, pval_w what dig_tiled_nb_test makes of those (NaN).
 * pt_w, k_w, exp_w, pval_w and n_windows may each be NULL and are then skipped.  DIG_TILE_WINDOW_MAX_WIDTH is the largest width (a
 * workgroup stages 1024 tiles and the width - 1 behind them in LDS).  DIG_EINVAL, before anything is read or launched, for a width
 * outside [1, DIG_TILE_WINDOW_MAX_WIDTH], C R >= 2^31, T >= 2^31 or more than 2^31 - 1 workgroups (C R ceil(T / 1024)).  Nothing is
 * launched or written -- n_windows neither -- when C R T = 0.  Every typed pointer needs the alignment of its element and no more. */
#define DIG_TILE_WINDOW_MAX_WIDTH 2048
int dig_tile_window_test(const double *pt, const int32_t *k, const double *mu, const double *sigma, const int32_t *n_valid, int64_t C,
                         int64_t R, int64_t T, int32_t width, double *pt_w, int32_t *k_w, double *exp_w, double *pval_w,
                         int32_t *n_windows, void *stream);
int dig_tile_window_test_host(const double *pt, const int32_t *k, const double *mu, const double *sigma, const int32_t *n_valid,
                              int64_t C, int64_t R, int64_t T, int32_t width, double *pt_w, int32_t *k_w, double *exp_w,
                              double *pval_w, int32_t *n_windows, int device);

/* ---- the distinct samples of sliding windows (additive: the ABI version stays) -------------------------------------- *
 * The samples of a window are not the sum of its tiles' samples: one sample with rows in several tiles of a window is one sample.
 * With n(c, r, t, s) the rows of global sample s that dig_tile_sample_keys counts in tile (c, r, t) -- the same skip rules, the same
 * keep -- and n_windows, "window t covers the tiles t .. min(t + width, nv) - 1", nv = min(n_valid[r], T) as dig_tile_window_test
 * defines them:
 *   s_w[c, r, t] = the samples s with n(c, r, u, s) > 0 for a tile u of window t      for t < n_windows[r], else 0.
 * The NB test of dig_tiled_nb_test on (pt_w, s_w, mu, sigma) is the window's PVAL_SAMPLE; width 1 gives k_samples of
 * dig_tile_sample_counts.
 *   dig_tile_window_sample_keys: the keys of dig_tile_sample_keys, ((row T + tile) << sb) | sample with row = cohort R + region and sb
 *     the bits that hold 0 .. n_samples, re-keyed sample-major: keys_out[i] = ((row << sb) | sample) T + tile, which fits 63 bits
 *     whenever the old key does.  A negative key, INT64_MAX and a key of a tile outside [0, C R T) become INT64_MAX.  keys i64 [n],
 *     sorted or not; keys_out i64 [n] may be keys.  One lane per key.
 *   The caller sorts keys_out ascending: the tiles of one sample in one row then lie next to each other, ascending.
 *   dig_tile_window_samples: s_w i32 [C, R, T] is zeroed; the head of every run of equal keys adds +1 at the first window in which its
 *     tile is the sample's first one, max(t_prev + 1, t - width + 1, 0) with t_prev the sample's previous tile in the row (the left
 *     neighbour of the head in keys_sorted, when it is of the same row and sample; else -1), and -1 one past the last such window,
 *     min(t + 1, n_windows[r]) (when that is below T); an in-place prefix sum along every row then gives the counts.  Two integer
 *     atomics per (tile, sample), however many rows it has; order-independent.  Keys that are negative, INT64_MAX, of a row >= C R or
 *     of a tile >= nv are passed over and never dereference anything.  n_valid i32 [R].
 * DIG_EINVAL, before anything is read or launched, for a width outside [1, DIG_TILE_WINDOW_MAX_WIDTH], C R >= 2^31, T >= 2^31,
 * n >= 2^31, C, R, T or n_samples at or above 2^31 and key fields that do not fit 63 bits.  Nothing is launched or written when
 * C R T = 0.  Every typed pointer needs the alignment of its element and no more.  The host twin of dig_tile_window_samples refuses
 * keys that are not ascending. */
int dig_tile_window_sample_keys(const int64_t *keys, int64_t n, int64_t C, int64_t R, int64_t T, int64_t n_samples, int64_t *keys_out,
                                void *stream);
int dig_tile_window_sample_keys_host(const int64_t *keys, int64_t n, int64_t C, int64_t R, int64_t T, int64_t n_samples,
                                     int64_t *keys_out, int device);
int dig_tile_window_samples(const int64_t *keys_sorted, int64_t n, const int32_t *n_valid, int64_t C, int64_t R, int64_t T,
                            int64_t n_samples, int32_t width, int32_t *s_w, void *stream);
int dig_tile_window_samples_host(const int64_t *keys_sorted, int64_t n, const int32_t *n_valid, int64_t C, int64_t R, int64_t T,
                                 int64_t n_samples, int32_t width, int32_t *s_w, int device);

/* ---- sliding windows over the mutated tiles only (additive: the ABI version stays) --------------------------------- *
 * dig_tile_window_test for the windows that hold a mutation row, and for no other, without a [C, R, T] plane.  Genome, chromosome
 * and region arguments, s_prob, n_up, binsize and n_tiles = T as dig_tile_census takes them; keys_sorted i64 [n]: the keys of
 * dig_sparse_tile_keys, (cohort R + region) T + tile, sorted ascending (a run of equal keys: a mutated tile); nv = min(n_valid[r], T)
 * and n_windows, "window w covers the tiles w .. min(w + width, nv) - 1" as dig_tile_window_test defines them.  A MUTATED WINDOW of
 * row (c, r) is a window w < n_windows[r] that covers a mutated tile of the row.  With t_prev the mutated tile in front of t in its
 * row (-1: none), tile t is the FIRST mutated tile of exactly the windows [lo, hi), lo = max(t_prev + 1, t - width + 1, 0),
 * hi = min(t + 1, n_windows[r]): every mutated window has one such tile and is named once, through it.
 *   dig_tile_window_census: n_windows i32 [R] (the bits of dig_tile_window_test) and n_positive_w i32 [C, R], the windows
 *     w < n_windows[r] that cover a tile with pt > 0 by the rule of dig_tile_census' n_positive -- the windows whose dense pt_w is > 0:
 *     for nv >= width, n_windows[r] minus the sum over the maximal runs of Z consecutive tiles without a positive position of
 *     max(Z - width + 1, 0); for 0 < nv < width, 1 when any tile is positive.  One workgroup per region, a pass per 64 cohorts;
 *     integers only, no atomics, the LDS use does not depend on T.  n_positive i32 [C, R] or NULL: the n_positive of dig_tile_census
 *     for the same binsize and n_tiles; a (region, pass of 64 cohorts) whose cohorts all have n_positive 0 or nv is then answered
 *     without walking the genome.  workspace: dig_tile_census_workspace(C, n_up) bytes, aligned to 8 bytes (the call fills it).
 *   dig_sparse_window_count: counts i64 [n]: at the head of a run max(hi - lo, 0), at every other index 0.  The head reads t_prev
 *     from its left neighbour (the same row iff prev / T == key / T).  Keys that are negative, INT64_MAX, of a row >= C R or of a tile
 *     >= nv get 0 before anything is dereferenced.  n_valid i32 [R].  One lane per key.
 *   The caller forms offsets i64 [n + 1], the exclusive prefix sum of counts with the total last (it may exceed 2^31).
 *   dig_sparse_window_test: the candidate windows j in [w_begin, w_begin + w_count) of the flat list, w_count < 2^31, one lane each.
 *     The owner is the last index i with offsets[i] <= j < offsets[i + 1]; the window is w = lo(i) + j - offsets[i]; out_k = (the
 *     first index at or behind i whose key is >= row T + min(w + width, nv)) - i; out_pt = (the sum of s_prob[c] over the window's
 *     positions in ascending order, valid contexts only, started at 0.0) / denom[c, r] -- ONE division: width 1 gives the seven
 *     outputs of dig_sparse_tile_test bit for bit, an aligned full window at (binsize, width) the pt bits of the sparse tile at
 *     binsize width; dig_tile_window_test adds the tiles' quotients instead and agrees to rounding (1e-12 relative), not in bits.
 *     out_exp = pt mu, out_pval: the device functions of dig_tiled_nb_test.  out_cohort, out_region, out_window, out_k i32, out_pt,
 *     out_exp, out_pval f64 [w_count], in the order of the list: cohort-major, then by region, then by window.  nv comes from the
 *     region table (what dig_tile_census writes as n_valid).  An index j that no head owns (offsets of another key list, a key
 *     outside [0, C R T)) gets cohort = region = window = -1, k = 0 and NaN: every element of the chunk is written.  denom, mu,
 *     sigma f64 [C, R].  Both genome walkers clamp every word index into [0, n_words).
 * DIG_EINVAL, before anything is read or launched, for a width outside [1, DIG_TILE_WINDOW_MAX_WIDTH], C R >= 2^31, C, R or T at or
 * above 2^31 and C R T beyond 62 bits.  Nothing is launched for R = 0 (census), n = 0 (count) or w_count = 0 (test).  Every typed
 * pointer needs the alignment of its element and no more.  The host twins refuse what the twins of dig_tile_census refuse of the
 * tables, keys that are not ascending and offsets that are not those of a prefix sum (0 first, non-decreasing). */
int dig_tile_window_census(const uint32_t *genome_words, int64_t n_words, const int64_t *chrom_off, const int64_t *chrom_len,
                           int n_chrom, const int32_t *reg_chrom, const int64_t *reg_start, const int64_t *reg_end, int64_t R,
                           const double *s_prob, int64_t C, int n_up, int binsize, int64_t n_tiles, int32_t width,
                           const int32_t *n_positive, int32_t *n_windows, int32_t *n_positive_w, void *workspace,
                           int64_t workspace_bytes, void *stream);
int dig_tile_window_census_host(const uint32_t *genome_words, int64_t n_words, const int64_t *chrom_off, const int64_t *chrom_len,
                                int n_chrom, const int32_t *reg_chrom, const int64_t *reg_start, const int64_t *reg_end, int64_t R,
                                const double *s_prob, int64_t C, int n_up, int binsize, int64_t n_tiles, int32_t width,
                                const int32_t *n_positive, int32_t *n_windows, int32_t *n_positive_w, int device);
int dig_sparse_window_count(const int64_t *keys_sorted, int64_t n, const int32_t *n_valid, int64_t C, int64_t R, int64_t T,
                            int32_t width, int64_t *counts, void *stream);
int dig_sparse_window_count_host(const int64_t *keys_sorted, int64_t n, const int32_t *n_valid, int64_t C, int64_t R, int64_t T,
                                 int32_t width, int64_t *counts, int device);
int dig_sparse_window_test(const uint32_t *genome_words, int64_t n_words, const int64_t *chrom_off, const int64_t *chrom_len,
                           int n_chrom, const int32_t *reg_chrom, const int64_t *reg_start, const int64_t *reg_end, int64_t R,
                           const double *s_prob, int64_t C, int n_up, int binsize, int64_t n_tiles, const double *denom,
                           const double *mu, const double *sigma, const int64_t *keys_sorted, int64_t n, const int64_t *offsets,
                           int32_t width, int64_t w_begin, int64_t w_count, int32_t *out_cohort, int32_t *out_region,
                           int32_t *out_window, int32_t *out_k, double *out_pt, double *out_exp, double *out_pval, void *stream);
int dig_sparse_window_test_host(const uint32_t *genome_words, int64_t n_words, const int64_t *chrom_off, const int64_t *chrom_len,
                                int n_chrom, const int32_t *reg_chrom, const int64_t *reg_start, const int64_t *reg_end, int64_t R,
                                const double *s_prob, int64_t C, int n_up, int binsize, int64_t n_tiles, const double *denom,
                                const double *mu, const double *sigma, const int64_t *keys_sorted, int64_t n, const int64_t *offsets,
                                int32_t width, int64_t w_begin, int64_t w_count, int32_t *out_cohort, int32_t *out_region,
                                int32_t *out_window, int32_t *out_k, double *out_pt, double *out_exp, double *out_pval, int device);

/* ---- sufficient statistics in canonical chunks (bin-sharded runs) --------------------------- *
 * Same quantity as dig_scale_suffstats / dig_scale_factors, defined so that it does not depend on the sharding: the bins
 * are cut into K canonical chunks of the GLOBAL grid (boundaries floor(N j / K)); a rank computes the chunk sums of the
 * chunks it owns (out_chunks [n_chunks, C], each in an order fixed by the chunk's rows and C alone), the chunk sums of
 * all ranks are all-gathered in chunk order and added first to last; obs f64 [world, 2, C] hold every rank's observed
 * SNV / indel counts (integers).  Bit-identical scale factors for any number of ranks.
 *   chunk_rows int64 [n_chunks + 1], HOST memory: first row of every chunk in this rank's table (+ end); n_chunks <= 256;
 *   C <= 256.  workspace: dig_scale_suffstats_chunked_workspace(chunk_rows, n_chunks, C) bytes, 8-byte aligned.
 *   bin_flag may be NULL (ABI 5): bin_mu then holds +0.0 in the flagged entries already (a plan-time copy saves the flag
 *   bytes of every step); the same additions, the same bits. */
int64_t dig_scale_suffstats_chunked_workspace(const int64_t *chunk_rows, int n_chunks, int64_t C);
int dig_scale_suffstats_chunked(const double *bin_mu, const uint8_t *bin_flag, int64_t C, const int64_t *chunk_rows,
                                int n_chunks, double *out_chunks, void *workspace, int64_t workspace_bytes, void *stream);
int dig_scale_factors_chunked(const double *chunk_sums, int n_chunks, const double *obs, int world, int64_t C,
                              double *out_sum, double *cj, double *cj_indel, void *stream);

/* ---- per-base / tiled route, front half -------------------------------------------------- *
 * base_probabilities_by_region (sequence_model/sequence_tools.py:292-317) + the tiling of apply_nb_to_region
 * (sequence_model/nb_model.py:126-186) for trinucleotide contexts (n_up = n_down = 1), all cohorts at once; the back
 * half is dig_tiled_nb_test.  Genome layout as dig_count_contexts.
 *   region r: positions max(start, 1) .. min(end, chrom_len - 1) - 1 (fetch_sequence :21-29); tile t = positions
 *       first + t * binsize .. (the last tile of a region may be shorter); n_valid[r] = number of tiles the region has
 *       (<= n_tiles), first_pos[r] = its first position.
 *   s_prob f64 [C, 64]: S_prob of cohort c by context index 16 b0 + 4 b1 + b2; a position whose window holds a non-ACGT
 *       base has probability 0.
 *   pt f64 [C, R, n_tiles]: (sum of S_prob over the tile's positions) / (sum over the region's positions); tiles past
 *       n_valid[r] are NaN.  Sums are regrouped by context (exact integer counts x table): a few ulp from the reference's
 *       normalise-then-np.sum order.
 * dig_tile_mut_counts: k i32 [C, R, n_tiles] (cleared by the call) from (mutation, region) pairs as produced by
 *   dig_overlap_join_count/fill with the regions as blocks: a pair counts when the mutation's START is one of the
 *   region's positions (value_counts of START, nb_model.py:135-136,160-163) in a tile below n_valid[region] and n_tiles;
 *   pairs whose mut_cohort is outside [0, C) are skipped. */
int dig_base_tile_probs(const uint32_t *genome_words, int64_t n_words, const int64_t *chrom_off, const int64_t *chrom_len,
                        int n_chrom, const int32_t *reg_chrom, const int64_t *reg_start, const int64_t *reg_end, int64_t R,
                        const double *s_prob, int64_t C, int binsize, int64_t n_tiles, double *pt, int64_t *first_pos,
                        int32_t *n_valid, void *stream);
int dig_tile_mut_counts(const int32_t *pair_mut, const int32_t *pair_reg, int64_t n_pairs, const int64_t *mut_start,
                        const int32_t *mut_cohort, const int64_t *first_pos, const int32_t *n_valid, int binsize,
                        int64_t n_tiles, int64_t R, int64_t C, int32_t *k, void *stream);
/* General-context form (ABI 4): n_up = n_down = 1 (forwards to dig_base_tile_probs) or 2 -- penta-nucleotide contexts, the
 * DEFAULT signature of the reference's per-base functions (sequence_tools.py:292, nb_model.py:126,188).  s_prob f64
 * [C, 4^(2 n_up + 1)] by context index (itertools.product('ACGT', repeat = 2 n_up + 1) order); positions
 * (start == 0 ? n_up : start) .. min(end, chrom_len - n_up) - 1 (fetch_sequence :21-29).  A region of more than 16 384
 * positions is NOT evaluated by the device entry point (n_valid[r] = -1, its pt NaN; ABI 6 -- before, such a region
 * overran a staging buffer); a caller that holds the coordinates on the host refuses such regions, and regions that
 * start inside (0, n_up), before the launch (the _host twin does).  Everything else as dig_base_tile_probs. */
int dig_base_tile_probs_ctx(const uint32_t *genome_words, int64_t n_words, const int64_t *chrom_off, const int64_t *chrom_len,
                            int n_chrom, const int32_t *reg_chrom, const int64_t *reg_start, const int64_t *reg_end, int64_t R,
                            const double *s_prob, int64_t C, int n_up, int binsize, int64_t n_tiles, double *pt,
                            int64_t *first_pos, int32_t *n_valid, void *stream);
int dig_base_tile_probs_ctx_host(const uint32_t *genome_words, int64_t n_words, const int64_t *chrom_off,
                                 const int64_t *chrom_len, int n_chrom, const int32_t *reg_chrom, const int64_t *reg_start,
                                 const int64_t *reg_end, int64_t R, const double *s_prob, int64_t C, int n_up, int binsize,
                                 int64_t n_tiles, double *pt, int64_t *first_pos, int32_t *n_valid, int device);
/* host twins (n_mut: rows of mut_start / mut_cohort, so that the twin knows how much to stage) */
int dig_base_tile_probs_host(const uint32_t *genome_words, int64_t n_words, const int64_t *chrom_off,
                             const int64_t *chrom_len, int n_chrom, const int32_t *reg_chrom, const int64_t *reg_start,
                             const int64_t *reg_end, int64_t R, const double *s_prob, int64_t C, int binsize, int64_t n_tiles,
                             double *pt, int64_t *first_pos, int32_t *n_valid, int device);
int dig_tile_mut_counts_host(const int32_t *pair_mut, const int32_t *pair_reg, int64_t n_pairs, const int64_t *mut_start,
                             int64_t n_mut, const int32_t *mut_cohort, const int64_t *first_pos, const int32_t *n_valid,
                             int binsize, int64_t n_tiles, int64_t R, int64_t C, int32_t *k, int device);

/* ---- per-cohort sufficient statistics for the scale factors --------------------------- *
 * calc_scale_factor_efficient, genome mode (driver_model/transfer_tools.py:148-156):
 *   out_sum[c] = sum over bins with FLAG == 0 of Y_PRED[bin, c]   (N_SNV_EXP per cohort);
 *   cj = N_SNV_OBS / out_sum, cj_indel = N_IND_OBS / out_sum are formed by the caller (after the
 *   all-gather of the per-shard sums when bins are sharded over GPUs).
 * bin_mu f64 [N, C], bin_flag u8 [N, C]; fixed summation order (bit-reproducible).
 * workspace: at least dig_scale_suffstats_workspace(N, C) bytes, 8-byte aligned. */
int64_t dig_scale_suffstats_workspace(int64_t N, int64_t C);
int dig_scale_suffstats(const double *bin_mu, const uint8_t *bin_flag, int64_t N, int64_t C, double *out_sum,
                        void *workspace, int64_t workspace_bytes, void *stream);
int dig_scale_suffstats_host(const double *bin_mu, const uint8_t *bin_flag, int64_t N, int64_t C, double *out_sum,
                             int device);

/* Scale factors from the (all-gathered) per-shard statistics, transfer_tools.py:153-154:
 *   parts f64 [world, 3, C]: row 0 = sum(Y_PRED[~FLAG]) of the shard, row 1 = its N_SNV_OBS, row 2 = its N_IND_OBS;
 *   cj[c] = sum_r parts[r][1][c] / sum_r parts[r][0][c],  cj_indel[c] = sum_r parts[r][2][c] / sum_r parts[r][0][c],
 *   both sums taken in rank order r = 0 .. world-1 (bit-reproducible on every rank).  world = 1: a plain division. */
int dig_scale_factors(const double *parts, int world, int64_t C, double *cj, double *cj_indel, void *stream);
/* Single-shard form of the two calls above (nothing to all-gather): out_sum as dig_scale_suffstats, and
 * cj[c] = n_snv_obs[c] / out_sum[c], cj_indel[c] = n_ind_obs[c] / out_sum[c] from the same final reduction kernel.
 * Same bits as dig_scale_suffstats + dig_scale_factors(world = 1).  Workspace as dig_scale_suffstats. */
int dig_scale_factors_local(const double *bin_mu, const uint8_t *bin_flag, int64_t N, int64_t C, const double *n_snv_obs,
                            const double *n_ind_obs, double *out_sum, double *cj, double *cj_indel, void *workspace,
                            int64_t workspace_bytes, void *stream);

/* ---- trinucleotide context counting from sequence ---------------------------------------- *
 * count_sequence_context over fetch_sequence (sequence_model/sequence_tools.py:21-29,42-55,65-80), for a batch of
 * regions: count_contexts_by_regions (:82-99), nonc_elt_context_count (:527-566), DIG_onthefly
 * (driver_model/onthefly_tools.py:70-71,120).
 *   genome_words u32 [n_words], 16-byte aligned (device entry point): 4 bits per base (A=0 C=1 G=2 T=3, anything else 4), 8 bases per word, base 0 in the
 *       low nibble; word 0 and word n_words-1 are all-N pad words; chromosome c occupies bases
 *       chrom_off[c] .. chrom_off[c] + chrom_len[c] - 1 counted from word 1, chrom_off[c] % 8 == 0.
 *   region r: centre positions max(start, 1) .. min(end, chrom_len - 1) - 1 of chromosome reg_chrom[r] (the fetch is
 *       widened by one base, START == 0 becomes 1, truncated at the chromosome end); a triplet holding a non-ACGT
 *       base is skipped; reg_minus[r] != 0 counts the reverse-complemented sequence ('-' strand elements).
 *   out i32 [R, 64], context index 16 b0 + 4 b1 + b2 (= itertools.product('ACGT', repeat=3) order).  Bit-exact. */
int dig_count_contexts(const uint32_t *genome_words, int64_t n_words, const int64_t *chrom_off,
                       const int64_t *chrom_len, int n_chrom, const int32_t *reg_chrom, const int64_t *reg_start,
                       const int64_t *reg_end, const uint8_t *reg_minus, int64_t R, int32_t *out, void *stream);
int dig_count_contexts_host(const uint32_t *genome_words, int64_t n_words, const int64_t *chrom_off,
                            const int64_t *chrom_len, int n_chrom, const int32_t *reg_chrom, const int64_t *reg_start,
                            const int64_t *reg_end, const uint8_t *reg_minus, int64_t R, int32_t *out, int device);

/* The same counts from the 2-BIT genome (ABI 6) -- half the bytes, no per-base test for unknown letters in the scan:
 *   words2 u32 [n_words2], 16-byte aligned: 2 bits per base (A=0 C=1 G=2 T=3; EVERY OTHER LETTER STORED AS A), 16 bases
 *       per word, base 0 in the low bits; array base g of chromosome position p is 64 + chrom_off[c] + p (64 pad bases
 *       = one 4-word group in front; chrom_off as above; at least 24 pad words behind the last chromosome).
 *   nint_start / nint_end i64 [n_int]: the maximal runs [start, end) of letters other than ACGT, in ARRAY bases, sorted,
 *       disjoint and not touching; nint_bucket i32 [n_buckets]: index of the first run that ends behind array base
 *       b << 12 (b = 0 .. n_buckets - 1, n_buckets > (last array base) >> 12).  n_int == 0: the three may be NULL.
 *   regions, strand flag and out exactly as dig_count_contexts; the same bits. */
int dig_count_contexts2(const uint32_t *words2, int64_t n_words2, const int64_t *nint_start, const int64_t *nint_end,
                        int64_t n_int, const int32_t *nint_bucket, int64_t n_buckets, const int64_t *chrom_off,
                        const int64_t *chrom_len, int n_chrom, const int32_t *reg_chrom, const int64_t *reg_start,
                        const int64_t *reg_end, const uint8_t *reg_minus, int64_t R, int32_t *out, void *stream);
int dig_count_contexts2_host(const uint32_t *words2, int64_t n_words2, const int64_t *nint_start, const int64_t *nint_end,
                             int64_t n_int, const int32_t *nint_bucket, int64_t n_buckets, const int64_t *chrom_off,
                             const int64_t *chrom_len, int n_chrom, const int32_t *reg_chrom, const int64_t *reg_start,
                             const int64_t *reg_end, const uint8_t *reg_minus, int64_t R, int32_t *out, int device);

/* Penta-nucleotide counts (n_up = n_down = 2) from the 2-bit genome of dig_count_contexts2 (same words2, run list, bucket
 * index, chromosome and region arrays):
 *   centres of region r run over [s, e) with s = 2 if START == 0 else START, e = min(END, chrom_len - 2) (the reference's
 *       fetch widened by two bases on either side, truncated at the chromosome end); an empty range gives a row of zeros;
 *       0 < START < 2 is refused (the _host twin returns DIG_EINVAL; the reference's fetch would start before base 0);
 *   a window holding any letter other than ACGT is skipped; reg_minus[r] != 0 counts the reverse-complemented sequence;
 *   out i32 [R, 1024], 16-byte aligned, context index 256 b0 + 64 b1 + 16 b2 + 4 b3 + b4 (= itertools.product('ACGT',
 *       repeat=5) order).  Counters are 32-bit: a region may be a whole chromosome. */
int dig_count_contexts5(const uint32_t *words2, int64_t n_words2, const int64_t *nint_start, const int64_t *nint_end,
                        int64_t n_int, const int32_t *nint_bucket, int64_t n_buckets, const int64_t *chrom_off,
                        const int64_t *chrom_len, int n_chrom, const int32_t *reg_chrom, const int64_t *reg_start,
                        const int64_t *reg_end, const uint8_t *reg_minus, int64_t R, int32_t *out, void *stream);
int dig_count_contexts5_host(const uint32_t *words2, int64_t n_words2, const int64_t *nint_start, const int64_t *nint_end,
                             int64_t n_int, const int32_t *nint_bucket, int64_t n_buckets, const int64_t *chrom_off,
                             const int64_t *chrom_len, int n_chrom, const int32_t *reg_chrom, const int64_t *reg_start,
                             const int64_t *reg_end, const uint8_t *reg_minus, int64_t R, int32_t *out, int device);

/* ---- sequence context of mutations (DigPreprocess.py addMutationContext) ------------------------------ *
 * mutation_contexts_by_chrom (sequence_model/sequence_tools.py:130-177) for rows in group order (chromosome-grouped; a run is a
 * maximal block of consecutive rows with the same chromosome and START), over the 2-bit genome of dig_count_contexts2 (words2,
 * the run list and its bucket index, chrom_off / chrom_len exactly as there):
 *   row_chrom i32 [n_rows] within [0, n_chrom); row_start i64 [n_rows] (0-based centre); row_ref u8 [n_rows]: 0-3 for a REF of one
 *       upper-case letter A C G T, 4 for a REF the caller found equal to a genome letter other than ACGT (such a row's window
 *       touches a non-ACGT run: DIG_MC_HOST), anything else never matches;
 *   window = bases START - n_up .. START + n_down, n_up, n_down >= 0, n_up + n_down + 1 <= 16;
 *   status u8 [n_rows]: DIG_MC_KEPT, DIG_MC_MISMATCH (seq[START] != REF), DIG_MC_DROPPED (it matches, an earlier row of its run
 *       does not), DIG_MC_HOST (it and its run match, but the window touches a letter other than ACGT, starts before the
 *       chromosome or is cut short at its end: the caller takes the letters from the FASTA); a START outside [0, chrom_len) is
 *       reported as DIG_MC_HOST with nothing read (the caller rejects it);
 *   context u32 [n_rows] (DIG_MC_KEPT rows): the window at 2 bits per base (A=0 C=1 G=2 T=3), window base k in bits 2 k, 2 k + 1;
 *       collapse != 0: reverse-complemented when the centre is A or G;
 *   workspace: dig_mutation_contexts_workspace(n_rows) bytes, 4-byte aligned.  n_rows < 2^31. */
#define DIG_MC_KEPT 0
#define DIG_MC_MISMATCH 1
#define DIG_MC_DROPPED 2
#define DIG_MC_HOST 3
int64_t dig_mutation_contexts_workspace(int64_t n_rows);
int dig_mutation_contexts(const uint32_t *words2, int64_t n_words2, const int64_t *nint_start, const int64_t *nint_end,
                          int64_t n_int, const int32_t *nint_bucket, int64_t n_buckets, const int64_t *chrom_off,
                          const int64_t *chrom_len, int n_chrom, const int32_t *row_chrom, const int64_t *row_start,
                          const uint8_t *row_ref, int64_t n_rows, int n_up, int n_down, int collapse, uint8_t *status,
                          uint32_t *context, void *workspace, int64_t workspace_bytes, void *stream);
int dig_mutation_contexts_host(const uint32_t *words2, int64_t n_words2, const int64_t *nint_start, const int64_t *nint_end,
                               int64_t n_int, const int32_t *nint_bucket, int64_t n_buckets, const int64_t *chrom_off,
                               const int64_t *chrom_len, int n_chrom, const int32_t *row_chrom, const int64_t *row_start,
                               const uint8_t *row_ref, int64_t n_rows, int n_up, int n_down, int collapse, uint8_t *status,
                               uint32_t *context, int device);

/* ---- genic function of mutations (DigPreprocess.py addMutationFunction; scripts/mutationFunction.R) ---- *
 * One work item is one (mutation, gene) pair of the interval join of the mutations with the genes' CDS blocks and
 * essential-splice positions, over the 2-bit genome of dig_count_contexts2 (words2, the run list and its bucket index,
 * chrom_off / chrom_len exactly as there).  All genome positions are 1-BASED and intervals closed.
 * Gene table (n_genes genes):
 *   gene_chrom i32 within [0, n_chrom); gene_minus u8 (1: the gene lies on the - strand);
 *   blk_ptr i64 [n_genes + 1], blk_start / blk_end i64 [blk_ptr[n_genes]]: the CDS blocks of gene g, ascending and disjoint;
 *   cds_off i64 per block: the CDS length in front of the block in genome order (the CDS length of a gene is a multiple of 3);
 *   spl_ptr i64 [n_genes + 1], spl_pos i64 [spl_ptr[n_genes]]: the essential-splice positions of gene g, ascending.
 * Pairs: pair_gene i32, pair_start / pair_end i64, pair_kind u8 (DIG_MF_KIND_*); SNVs: pair_ref / pair_alt u8, the codes 0-3
 *   (A C G T) of REF and ALT on the + strand (anything else in pair_ref never matches; pair_alt is taken modulo 4).
 * Outputs per pair:
 *   SNV (pos = pair_start): impact = DIG_MF_SPLICE when pos is a splice position of the gene; otherwise pos_ind, the 1-based index
 *     of pos in the CDS read in transcript direction, its codon (CDS positions 3 ceil(pos_ind / 3) - 2 .. 3 ceil(pos_ind / 3), which
 *     may lie in up to three blocks; complemented for a - gene) and the codon with ALT in place go through the standard genetic
 *     code: same amino acid DIG_MF_SYN, else new stop DIG_MF_NONS, else old not stop DIG_MF_MIS, else DIG_MF_STOP_LOSS.
 *     n_cds = 1, cds_min = cds_max = pos_ind (n_cds = 0 for a splice position).
 *     status: DIG_MF_OK; DIG_MF_WRONG_REF (the genome base at pos is not REF; impact is still that of ALT on the genome's codon);
 *     DIG_MF_HOST (pos or a base of the codon is a letter other than ACGT: impact = DIG_MF_NONE, the caller finishes the pair
 *     from the letters);
 *     DIG_MF_OUTSIDE (pos is neither in a CDS block nor a splice position of the gene, or the gene index is out of range).
 *   other kinds: impact = DIG_MF_NONE, status = DIG_MF_OK; n_cds, cds_min, cds_max = count, minimum and maximum of the CDS
 *     indices (transcript direction) of the positions pair_start .. pair_end (DIG_MF_KIND_INS: pair_start - 1 .. pair_end) that lie
 *     in the gene's CDS blocks; no genome read.  n_cds = 0 (cds_min = cds_max = 0) when no position does. */
#define DIG_MF_KIND_SNV 0
#define DIG_MF_KIND_INS 1
#define DIG_MF_KIND_OTHER 2
#define DIG_MF_SYN 0
#define DIG_MF_MIS 1
#define DIG_MF_NONS 2
#define DIG_MF_STOP_LOSS 3
#define DIG_MF_SPLICE 4
#define DIG_MF_NONE 255
#define DIG_MF_OK 0
#define DIG_MF_WRONG_REF 1
#define DIG_MF_HOST 2
#define DIG_MF_OUTSIDE 3
int dig_mutation_function(const uint32_t *words2, int64_t n_words2, const int64_t *nint_start, const int64_t *nint_end,
                          int64_t n_int, const int32_t *nint_bucket, int64_t n_buckets, const int64_t *chrom_off,
                          const int64_t *chrom_len, int n_chrom, const int32_t *gene_chrom, const uint8_t *gene_minus,
                          const int64_t *blk_ptr, const int64_t *blk_start, const int64_t *blk_end, const int64_t *cds_off,
                          const int64_t *spl_ptr, const int64_t *spl_pos, int64_t n_genes, const int32_t *pair_gene,
                          const int64_t *pair_start, const int64_t *pair_end, const uint8_t *pair_kind, const uint8_t *pair_ref,
                          const uint8_t *pair_alt, int64_t n_pairs, uint8_t *impact, uint8_t *status, int32_t *n_cds,
                          int32_t *cds_min, int32_t *cds_max, void *stream);
int dig_mutation_function_host(const uint32_t *words2, int64_t n_words2, const int64_t *nint_start, const int64_t *nint_end,
                               int64_t n_int, const int32_t *nint_bucket, int64_t n_buckets, const int64_t *chrom_off,
                               const int64_t *chrom_len, int n_chrom, const int32_t *gene_chrom, const uint8_t *gene_minus,
                               const int64_t *blk_ptr, const int64_t *blk_start, const int64_t *blk_end, const int64_t *cds_off,
                               const int64_t *spl_ptr, const int64_t *spl_pos, int64_t n_genes, const int32_t *pair_gene,
                               const int64_t *pair_start, const int64_t *pair_end, const uint8_t *pair_kind,
                               const uint8_t *pair_ref, const uint8_t *pair_alt, int64_t n_pairs, uint8_t *impact, uint8_t *status,
                               int32_t *n_cds, int32_t *cds_min, int32_t *cds_max, int device);

/* ---- possible substitutions of genes (DigPreprocess.py preprocess_genic_model --cds-bed: the L of the gene container) ---- *
 * For every gene of the gene table of dig_mutation_function (same ten genome arguments, same eight gene-table arguments, no
 * pairs) the number of possible single-base substitutions by effect class and substitution type:
 *   L i32 [n_genes, 4, 192]: class 0 silent, 1 missense, 2 nonsense, 3 essential splice (the rows of the reference's L_data,
 *       genic_driver_tools.py:110-123).  Every CDS base p (CDS index 1 .. len in transcript direction) and each of its three
 *       alternates is classified on its codon as dig_mutation_function classifies an SNV; DIG_MF_SYN / _MIS / _NONS add one to class
 *       0 / 1 / 2, DIG_MF_STOP_LOSS to none (it is counted in n_stop_loss).  Every splice position adds its three alternates to
 *       class 3.
 *   type: the genome's bases p - 1, p, p + 1 (at an exon edge a flank is an intron base) in transcript direction -- reverse-
 *       complemented for a - gene, the alternate complemented -- as X Y Z -> X a Z with A C G T = 0 .. 3: column
 *       3 (16 X + 4 Y + Z) + rank of a among the three bases other than Y (the sorted substitution index, mk_trans_idx).
 *   n_stop_loss i32 [n_genes]; status u8 [n_genes]: DIG_GS_OK, or DIG_GS_HOST for a gene in which a base read (a CDS or splice
 *       position or a flank) is a letter other than ACGT or lies outside the chromosome: its L row and n_stop_loss are zero and
 *       the caller finishes it from the letters.  Every output row is written (nothing to zero beforehand). */
#define DIG_GS_OK 0
#define DIG_GS_HOST 1
int dig_gene_site_counts(const uint32_t *words2, int64_t n_words2, const int64_t *nint_start, const int64_t *nint_end,
                         int64_t n_int, const int32_t *nint_bucket, int64_t n_buckets, const int64_t *chrom_off,
                         const int64_t *chrom_len, int n_chrom, const int32_t *gene_chrom, const uint8_t *gene_minus,
                         const int64_t *blk_ptr, const int64_t *blk_start, const int64_t *blk_end, const int64_t *cds_off,
                         const int64_t *spl_ptr, const int64_t *spl_pos, int64_t n_genes, int32_t *L, int32_t *n_stop_loss,
                         uint8_t *status, void *stream);
int dig_gene_site_counts_host(const uint32_t *words2, int64_t n_words2, const int64_t *nint_start, const int64_t *nint_end,
                              int64_t n_int, const int32_t *nint_bucket, int64_t n_buckets, const int64_t *chrom_off,
                              const int64_t *chrom_len, int n_chrom, const int32_t *gene_chrom, const uint8_t *gene_minus,
                              const int64_t *blk_ptr, const int64_t *blk_start, const int64_t *blk_end, const int64_t *cds_off,
                              const int64_t *spl_ptr, const int64_t *spl_pos, int64_t n_genes, int32_t *L, int32_t *n_stop_loss,
                              uint8_t *status, int device);

/* ---- context counts of bed12 elements (cohort_batch.run_quick_cohorts: the L of ad-hoc elements) ---------- *
 * The strand-aware trinucleotide counts of E elements straight from the 2-bit genome of dig_count_contexts2 (the same ten
 * genome arguments):
 *   elt_chrom i32 [E]; elt_minus u8 [E] (non-zero: the element lies on the - strand);
 *   blk_ptr i64 [E + 1], non-decreasing from 0 to n_blocks; blk_start / blk_end i64 [n_blocks]: the blocks of element e are
 *       blk_ptr[e] .. blk_ptr[e + 1] - 1, in any order, overlapping or repeated as the bed file has them;
 *   out i32 [E, 64], 4-byte aligned, context index 16 b0 + 4 b1 + b2: out[e] = the sum over the blocks b of element e of the row
 *       dig_count_contexts2 gives for (elt_chrom[e], blk_start[b], blk_end[b], elt_minus[e]): centres max(start, 1) ..
 *       min(end, chrom_len - 1) - 1, a triplet holding a letter other than ACGT skipped, the reverse complement for a - element;
 *       a block listed twice counts twice; an element without blocks and an empty or inverted block give zeros.  Every row is
 *       written (zeroed, then added to).  Integer counts: bit-exact whatever the mapping.
 *   workspace: dig_element_context_counts_workspace(n_blocks) bytes, 8-byte aligned (the list of the blocks that are cut
 *       across waves).  E, n_blocks < 2^31.
 * The device entry point cannot see its device arrays: a chromosome id outside [0, n_chrom) counts nothing there and a blk_ptr
 * that is not as stated gives unspecified counts (nothing outside the arrays is read or written); the _host twin refuses both
 * with DIG_EINVAL, as it refuses negative coordinates and blk_ptr[E] != n_blocks. */
int64_t dig_element_context_counts_workspace(int64_t n_blocks);
int dig_element_context_counts(const uint32_t *words2, int64_t n_words2, const int64_t *nint_start, const int64_t *nint_end,
                               int64_t n_int, const int32_t *nint_bucket, int64_t n_buckets, const int64_t *chrom_off,
                               const int64_t *chrom_len, int n_chrom, const int32_t *elt_chrom, const uint8_t *elt_minus,
                               const int64_t *blk_ptr, const int64_t *blk_start, const int64_t *blk_end, int64_t E,
                               int64_t n_blocks, int32_t *out, void *workspace, int64_t workspace_bytes, void *stream);
int dig_element_context_counts_host(const uint32_t *words2, int64_t n_words2, const int64_t *nint_start, const int64_t *nint_end,
                                    int64_t n_int, const int32_t *nint_bucket, int64_t n_buckets, const int64_t *chrom_off,
                                    const int64_t *chrom_len, int n_chrom, const int32_t *elt_chrom, const uint8_t *elt_minus,
                                    const int64_t *blk_ptr, const int64_t *blk_start, const int64_t *blk_end, int64_t E,
                                    int64_t n_blocks, int32_t *out, int device);

/* ---- result files (ABI 6; host code only) ------------------------------------------------- *
 * The text DataFrame.to_csv(path, header=True, index=True, sep="\t") writes for a frame (DigDriver.py:115-118): `header`
 * (a complete first line, no newline), then n_rows rows  label TAB col_0 TAB ... col_{n_cols-1}.
 *   labels: the row labels as one UTF-8 blob, label r = bytes label_off[r] .. label_off[r + 1] - 1;
 *   col_kind[j]: 0 = float64, written as Python's repr (shortest round-trip digits; positional for 1e-4 <= |x| < 1e16, else
 *       d.ddde-XX; NaN = empty field, inf / -inf), 1 = int64, 2 = bool as uint8 (True / False);
 *   n_threads: rows are formatted by up to 16 threads and written in order. */
int dig_write_tsv_host(const char *path, const char *header, const char *labels, const int64_t *label_off, int64_t n_rows,
                       int n_cols, const void *const *col_ptr, const int *col_kind, int n_threads);

/* ---- annotated mutation files (ABI 7; host code only) -------------------------------------- *
 * What mutation_tools.read_mutation_file (mutation_tools.py:45-104) + the encoding of the many-cohort driver do for one file
 * (tab-separated, no header: CHROM START END REF ALT SAMPLE GENE ANNOT [...]), without the interpreter:
 *   rows whose CHROM (one leading "chr" removed) is not "1" .. "22" are dropped; sample = id in order of first appearance
 *   among the kept rows; gene = id in order of first appearance in the file; indel = (ANNOT == "INDEL"); uid = dense rank of
 *   (CHROM, START, END, REF, ALT) among the kept rows (REF / ALT compared as ids of first appearance).
 * parse: *n_rows = kept rows, *n_samples, *names_bytes = length of the '\n'-joined sample names; *n_rows = -1 and no handle
 *   when the file holds something the parser does not cover (a double quote, a non-integer coordinate, ragged rows): the
 *   caller parses such a file as before.  fetch: copies the seven int64 columns and the names into the caller's buffers.
 *   free: releases the handle (NULL allowed). */
int dig_mutation_file_parse_host(const char *path, void **handle, int64_t *n_rows, int64_t *n_samples, int64_t *names_bytes);
int dig_mutation_file_fetch_host(void *handle, int64_t *chrom, int64_t *start, int64_t *end, int64_t *uid, int64_t *sample,
                                 int64_t *indel, int64_t *gene, char *sample_names);
/* flags (round 5): the reference's two de-duplications of a cohort's rows -- drop_duplicate_mutations, then get_unique_indels
 * (mutation_tools.py:106-117) -- as per-row 0 / 1 flags in file order: first_row[i] = no earlier row has the same mutation and
 * sample; first_indel[i] = row i is such a row, is an INDEL, and no earlier such row has the same mutation and GENE label.  The
 * genome-mode scale factors (calc_scale_factor_efficient, transfer_tools.py:129-159) count flagged rows: no sort on the device. */
int dig_mutation_file_flags_host(void *handle, int64_t *first_row, int64_t *first_indel);
int dig_mutation_file_free_host(void *handle);

/* ---- raw mutation calls -> annotated file (addMutationContext, DigPreprocess.py:75-100; host code only) ---------- *
 * For an 8-column file (CHROM START END REF ALT SAMPLE GENE ANNOT) that pandas would echo unchanged -- no NaN spelling, quote,
 * CR, NUL or non-ASCII byte, 8 fields on every line, no empty line, START / END canonical integers -- what read_mutation_file +
 * add_context_to_mutations + to_csv(sep="\t", index=False, header=False) write:
 * parse: *n_snv = rows of the SNV branch (CHROM exactly "1" .. "22", ANNOT not containing "INDEL", grouped by CHROM, file order
 *   inside), *n_indel = rows of the indel branch (after the de-duplication of ANNOT == "INDEL" rows on CHROM START END REF ALT
 *   GENE); *n_snv = -1 and no handle for any other file (the caller takes the pandas path).
 * fetch: the SNV rows' CHROM (1 .. 22), START and REF code: 0-3 for one upper-case ACGT letter, the byte itself for one
 *   other letter (the caller compares it with the genome: 4 or 255 for dig_mutation_contexts), 255 otherwise.
 * write: status / context of dig_mutation_contexts for the n_snv rows; host_text / host_off [n_host + 1]: the contexts of the
 *   DIG_MC_HOST rows, in row order (an empty one drops the row).  Kept SNV rows get MUT_TYPE = REF>ALT and CONTEXT; indel rows
 *   ANNOT "INDEL", their ANNOT as MUT_TYPE and CONTEXT "."; with any indel row the output is stably sorted by (CHROM, START, END).
 * free: releases the handle (NULL allowed). */
int dig_mutctx_file_parse_host(const char *path, void **handle, int64_t *n_snv, int64_t *n_indel);
int dig_mutctx_file_fetch_host(void *handle, int32_t *chrom, int64_t *start, uint8_t *ref);
int dig_mutctx_file_write_host(void *handle, const char *path, const uint8_t *status, const uint32_t *context,
                               const char *host_text, const int64_t *host_off, int n_up, int n_down);
int dig_mutctx_file_free_host(void *handle);

/* ---- Benjamini-Hochberg q-values (nb_model.get_q_vals, nb_model.py:340-342 = statsmodels fdrcorrection, method 'indep') ---- *
 * For `rows` lists of n p-values each, every list ALREADY in ascending order (the caller sorts: torch.sort / rocPRIM; row r at
 * p_sorted + r n): q_sorted[i] = min(1, min_{j >= i} p[j] / ((j + 1) / n)), the same IEEE operations in the same order as the host
 * form (a NaN -- sorted last -- makes every q of its list NaN, as statsmodels does).  workspace: dig_bh_workspace(n, rows) bytes, 8-byte aligned.  One HBM-bound pass (round 5: torch.cummin took 21 ms per 7.2 M values, 99 % of the
 * per-base route of BASELINE configs[4]). */
int64_t dig_bh_workspace(int64_t n, int64_t rows);
int dig_bh_qvalues_sorted(const double *p_sorted, int64_t n, int64_t rows, double *q_sorted, void *workspace, int64_t workspace_bytes,
                          void *stream);
/* Ranking p-values on the device (ABI 11, round 6; csrc/dig_sort.hip): a batched LSD radix sort written for this step (63-bit
 * keys in 9-bit digits, four passes over the upper 36 bits + a fix-up of the short runs that share them; ranges of 65 536
 * elements: histogram, scan, scatter -- no workgroup waits for another one) with the Benjamini-Hochberg pass behind it -- what
 * nb_model.get_q_vals (nb_model.py:340-342) needs for every cohort of the per-base route at once.
 *   rows: ragged lists in one array, row r = elements row_ptr[r] .. row_ptr[r + 1] - 1 (row_ptr: HOST array of rows + 1 offsets;
 *       a row holds fewer than 2^30 elements).  p, q, p_sorted, order: DEVICE arrays indexed like p.
 *   dig_sort_rows: p_sorted = the row's values ascending (every NaN last), order[j] = position in the row of the j-th smallest;
 *       either may be NULL.
 *   dig_bh_qvalues_ragged: q[i] = Benjamini-Hochberg q-value of p[i] among its row (statsmodels' operations, the bits of
 *       dig_bh_qvalues_sorted behind a stable sort; equal p-values have equal q-values, so the order among them is free).
 *       n_global, rank0, carry (HOST arrays of `rows`, each may be NULL): the row is the ranks rank0[r] + 1 .. of a list of
 *       n_global[r] values whose elements behind the row have the running minimum carry[r] (+inf when NULL) -- a rank of a
 *       sample sort finishes its range of the global order with them.  row_min (DEVICE, `rows`, may be NULL): the minimum of
 *       p / (rank / n) over the row, without carry (what the ranks in front take as their carry).  q may be NULL when only
 *       row_min is wanted.  sorted_out != 0: q leaves in ascending order of p instead of in place.
 *       The way back to the elements' places: q is a step function of p (one step per record of the reverse running minimum),
 *       so only the keys are sorted, the records go into a table per row and every element finds its q by its own value; a row
 *       with more records than half its length makes the call sort again with a 32-bit payload and write q through it.  The
 *       call synchronises `stream` (row tables go up, one flag word comes back).
 *   workspace: dig_bh_ragged_workspace(row_ptr, rows) bytes (24.2 bytes per element + tables) at any alignment: the calls lay
 *       their tables out from the next 256-byte boundary inside it, and the query includes that slack. */
int64_t dig_bh_ragged_workspace(const int64_t *row_ptr, int64_t rows);
int dig_sort_rows(const double *p, const int64_t *row_ptr, int64_t rows, double *p_sorted, uint32_t *order, void *workspace,
                  int64_t workspace_bytes, void *stream);
int dig_bh_qvalues_ragged(const double *p, const int64_t *row_ptr, int64_t rows, const double *n_global, const int64_t *rank0,
                          const double *carry, double *q, double *row_min, int sorted_out, void *workspace, int64_t workspace_bytes,
                          void *stream);

/* get_ideal_overlaps(chrom, intervals, window)  genic_driver_tools.py:275-283, for a batch of
 * elements (host-side index construction, integer only): block b of element e covers bins
 * floor(start/w)*w ... ceil(end/w)*w; duplicates removed; rows are looked up in the sorted bin
 * table (bin_chrom, bin_start) of N rows.  Two-call protocol: with ov_idx == NULL only ov_ptr
 * (E+1) is filled so the caller can size ov_idx = ov_ptr[E].  A bin that is not in the table
 * is an error (the reference raises KeyError at df.loc, genic_driver_tools.py:265). */
int dig_ideal_overlaps_host(const int32_t *elt_chrom, const int64_t *blk_ptr, const int64_t *blk_start,
                            const int64_t *blk_end, int64_t E, int64_t window, const int32_t *bin_chrom,
                            const int64_t *bin_start, int64_t N, int64_t *ov_ptr, int32_t *ov_idx);

/* ---- mutation x element-block interval join (data_tools/mutation_tools.py:191-230) ----------- *
 * Replaces `bedtools intersect -wa -wb` of the mutation file with the bed6 blocks of the elements: half-open
 * overlap  m.start < b.end && b.start < m.end  on the same chromosome (a zero-length mutation is tested as
 * [start, start+1)).  Blocks are sorted by (chrom, start) and given as composite keys:
 *   blk_start_key[i] = chrom << 40 | start,  blk_runmax_key[i] = chrom << 40 | running max of end within the chrom,
 *   blk_end[i] = end.   Mutations: mut_chrom, mut_start, mut_end (int64, any order).
 * Two-call protocol: dig_overlap_join_count fills counts[n_mut] (overlapped blocks per mutation); the caller
 * forms the exclusive prefix sum `offsets`; dig_overlap_join_fill writes the pairs (mutation row, block row) at
 * offsets[m] ..., mutation-major with blocks ascending -- the order bedtools reports them in.  The integer
 * bookkeeping after the join (de-duplication, per-sample caps, blacklist; :208-226, :155-189) is sort/unique work. */
int dig_overlap_join_count(const int64_t *blk_start_key, const int64_t *blk_runmax_key, const int64_t *blk_end,
                           int64_t n_blk, const int64_t *mut_chrom, const int64_t *mut_start, const int64_t *mut_end,
                           int64_t n_mut, int32_t *counts, void *stream);
int dig_overlap_join_fill(const int64_t *blk_start_key, const int64_t *blk_runmax_key, const int64_t *blk_end,
                          int64_t n_blk, const int64_t *mut_chrom, const int64_t *mut_start, const int64_t *mut_end,
                          int64_t n_mut, const int64_t *offsets, int32_t *pair_mut, int32_t *pair_blk, void *stream);
/* host twins (n_pairs = offsets[n_mut - 1] + counts[n_mut - 1]: the size of pair_mut / pair_blk) */
int dig_overlap_join_count_host(const int64_t *blk_start_key, const int64_t *blk_runmax_key, const int64_t *blk_end,
                                int64_t n_blk, const int64_t *mut_chrom, const int64_t *mut_start, const int64_t *mut_end,
                                int64_t n_mut, int32_t *counts, int device);
int dig_overlap_join_fill_host(const int64_t *blk_start_key, const int64_t *blk_runmax_key, const int64_t *blk_end,
                               int64_t n_blk, const int64_t *mut_chrom, const int64_t *mut_start, const int64_t *mut_end,
                               int64_t n_mut, const int64_t *offsets, int64_t n_pairs, int32_t *pair_mut, int32_t *pair_blk,
                               int device);

/* ---- per-bin epigenomic-track gather (region_model/data_aux/mut_dataset.py:76-81) ---- *
 * out[b, l, t] = (float) x_data[bin_rows[b], l, tracks[t]]      (transpose_out == 0)
 * out[b, t, l] = ...                                            (transpose_out != 0: the
 *   channels-first layout SimpleMultiTaskResNet.forward makes with transpose(x, 1, 2),
 *   region_model/nets/cnn_predictors.py:131)
 * x_data is [N, L, T] of src_dtype (DIG_F32 | DIG_F64 | DIG_I16); out is DIG_F32 or DIG_BF16.
 * tracks == NULL selects all tracks in order (T_sel must equal T; the reference's default when no track file is
 * given, dataset_generator.py:52-55): a bin is then one contiguous block and is copied with 8 / 16-byte accesses. */
int dig_gather_bins(const void *x_data, int src_dtype, int64_t N, int64_t L, int64_t T, const int64_t *bin_rows,
                    int64_t B, const int32_t *tracks, int64_t T_sel, void *out, int out_dtype, int transpose_out,
                    void *stream);
int dig_gather_bins_host(const void *x_data, int src_dtype, int64_t N, int64_t L, int64_t T, const int64_t *bin_rows,
                         int64_t B, const int32_t *tracks, int64_t T_sel, void *out, int out_dtype, int transpose_out,
                         int device);

/* ---- per-base tiled NB test (nb_model.py:126-186, arithmetic of apply_nb_to_region) --- *
 * For cohort c, bin b, tile t:  alpha, theta = normal_params_to_gamma(mu[c,b], sigma[c,b]);
 *   p = 1/(pt * theta + 1);  pval = nb_pvalue_exact(k, alpha, p);  exp = pt * mu   (:141-178)
 * pt f64 [C or 1, n_bins, n_tiles] (pt_per_cohort selects), k i32 [C, n_bins, n_tiles],
 * mu, sigma f64 [C, n_bins]; pval, exp f64 [C, n_bins, n_tiles]. */
int dig_tiled_nb_test(const double *pt, int pt_per_cohort, const int32_t *k, const double *mu, const double *sigma,
                      double *pval, double *exp_out, int64_t C, int64_t n_bins, int64_t n_tiles, void *stream);
int dig_tiled_nb_test_host(const double *pt, int pt_per_cohort, const int32_t *k, const double *mu,
                           const double *sigma, double *pval, double *exp_out, int64_t C, int64_t n_bins,
                           int64_t n_tiles, int device);

/* ---- RBF cross-covariance of the sparse-GP calibration (gp_trainer.py:28-45: ScaleKernel(RBFKernel) between the m
 * inducing points and the n training rows) as single passes over the m x n matrix ----------------------------------- *
 * dig_rbf_cross: K[i][j] = outputscale * exp(-|z_i - x_j|^2 / (2 lengthscale^2)), Z f64 [m, d], X f64 [n, d], d <= 32,
 *   K f64 [m, n] row-major.
 * dig_rbf_backward: W = g o K and, per row and 1024-column chunk, partial[row][chunk] = {sum W, sum W d2}
 *   (dig_rbf_backward_partials(m, n) doubles; summed by the caller: d outputscale = sum W / outputscale,
 *   d lengthscale = sum W d2 / lengthscale^3, dZ = (W X - rowsum(W) o Z) / lengthscale^2). */
int dig_rbf_cross(const double *Z, const double *X, int64_t m, int64_t n, int64_t d, double lengthscale, double outputscale,
                  double *K, void *stream);
int64_t dig_rbf_backward_partials(int64_t m, int64_t n);
int dig_rbf_backward(const double *g, const double *K, int64_t m, int64_t n, double lengthscale, double outputscale,
                     double *W, double *partial, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DIG_HIP_H */
