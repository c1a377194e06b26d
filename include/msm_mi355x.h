/*
 * msm_mi355x.h -- C ABI of the MI355X (gfx950) BLS12-381 MSM engine
 * (libmsm_mi355x.so, built from msm_blst_amd/csrc).
 *
 * Drop-in boundary for the hot path of LuoGuiwen/MSM_blst (a blst v0.3.10
 * fork): plain C types and pointers only, layout-identical to
 * bindings/blst.h, so a caller of the reference links this library for the
 * MSM entry points below instead of libblst's.  Each declaration cites the
 * reference interface it replaces.
 *
 * Threading: entry points are thread-safe per call (each blst-named call leases
 * an engine with its own device buffers and stream from a process-wide pool;
 * engine contexts are not shared across threads unless the
 * caller serialises).  Errors: the blst-named functions keep blst's void
 * signatures; by default a HIP failure inside one prints the error and aborts
 * (a silent wrong answer is never returned); after msm_set_abort_on_error(0)
 * such a call returns with its result set to the all-zero point (infinity;
 * blst_p{1,2}s_mult_wbits_precompute: the whole table zeroed, never half written),
 * msm_error_pending() nonzero and the message in msm_last_error().  The msm_*
 * extension API returns MSM_OK or a negative MSM_E* code and msm_last_error()
 * describes it.
 */
#ifndef MSM_MI355X_H
#define MSM_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- types: layout-identical to /root/reference/bindings/blst.h ---- */
typedef uint8_t byte;                                      /* blst.h:53 */
typedef uint64_t limb_t;                                   /* blst.h:54 */
typedef struct { byte b[256 / 8]; } blst_scalar;           /* blst.h:56 */
typedef struct { limb_t l[384 / 8 / sizeof(limb_t)]; } blst_fp;  /* blst.h:58 */
typedef struct { blst_fp fp[2]; } blst_fp2;                /* blst.h:60 */
typedef struct { blst_fp x, y, z; } blst_p1;               /* blst.h:164 */
typedef struct { blst_fp x, y; } blst_p1_affine;           /* blst.h:165 */
typedef struct { blst_fp2 x, y, z; } blst_p2;              /* blst.h:191 */
typedef struct { blst_fp2 x, y; } blst_p2_affine;          /* blst.h:192 */
typedef struct { blst_fp x, y, zzz, zz; } blst_p1xyzz;     /* blst.h:251 */
typedef struct { blst_fp2 x, y, zzz, zz; } blst_p2xyzz;    /* blst.h:252 */
typedef struct { int m; int b; int alpha; } digit_decomposition; /* blst.h:253 */

/* ---- plain Pippenger (replaces src/multi_scalar.c:581-607, blst.h:238-246, :377-384) ----
 * Same semantics as blst: points[] / scalars[] are arrays of pointers; when
 * points[1] (resp. scalars[1]) is NULL the data is one flat array, scalars
 * packed with stride (nbits+7)/8 (multi_scalar.c:393-416).  The low nbits bits
 * of each scalar are used (scalars are not reduced mod r).  The all-zero
 * affine point is infinity and contributes nothing.  ret is a Jacobian point
 * in Montgomery form; any representative (callers normalise with to_affine).
 * scratch is accepted for ABI compatibility and not used (device buffers are
 * the engine's own).  Unlike blst (defect at n=1), any n >= 0 is exact. */
size_t blst_p1s_mult_pippenger_scratch_sizeof(size_t npoints);
void blst_p1s_mult_pippenger(blst_p1 *ret, const blst_p1_affine *const points[], size_t npoints,
                             const byte *const scalars[], size_t nbits, limb_t *scratch);
void blst_p1s_tile_pippenger(blst_p1 *ret, const blst_p1_affine *const points[], size_t npoints,
                             const byte *const scalars[], size_t nbits, limb_t *scratch, size_t bit0,
                             size_t window);
size_t blst_p2s_mult_pippenger_scratch_sizeof(size_t npoints);
void blst_p2s_mult_pippenger(blst_p2 *ret, const blst_p2_affine *const points[], size_t npoints,
                             const byte *const scalars[], size_t nbits, limb_t *scratch);
void blst_p2s_tile_pippenger(blst_p2 *ret, const blst_p2_affine *const points[], size_t npoints,
                             const byte *const scalars[], size_t nbits, limb_t *scratch, size_t bit0,
                             size_t window);

/* ---- blst-level CHES / BGMW95 entry points (replace ref src/multi_scalar.c:584-790,
 * declared at ref bindings/blst.h:249-357; used by ref main_p1.cpp:233-236, :279-282, :384) ----
 * Same names, argument meaning and layouts.  The tile_* and integrate_* calls run on
 * the GPU (entries uploaded, sorted by bucket, accumulated one lane per bucket, then
 * the weighted bucket sum); the per-point helpers run on the host (one point op is
 * far below a kernel launch).  Differences, all toward the mathematically exact sum:
 * the last-element guard of ref multi_scalar.c:461 is applied to the last element's
 * own bucket (SURVEY 8a defect 1); buckets[] is filled with the per-bucket sums as
 * the reference leaves it (xyzz representatives may differ; equal as points). */
size_t blst_p1s_mult_pippenger_scratch_sizeof_CHES(size_t window);  /* multi_scalar.c:584-585 */
size_t blst_p2s_mult_pippenger_scratch_sizeof_CHES(size_t window);
void blst_p1xyzz_dadd_affine(blst_p1xyzz *out, const blst_p1xyzz *in, const blst_p1_affine *p,
                             unsigned char booth_sign);              /* ec_ops.h:710-769 */
void blst_p2xyzz_dadd_affine(blst_p2xyzz *out, const blst_p2xyzz *in, const blst_p2_affine *p,
                             unsigned char booth_sign);
void blst_p1xyzz_dadd(blst_p1xyzz *p3, const blst_p1xyzz *p1, const blst_p1xyzz *p2);  /* ec_ops.h:642-702 */
void blst_p2xyzz_dadd(blst_p2xyzz *p3, const blst_p2xyzz *p1, const blst_p2xyzz *p2);
void blst_p1xyzz_to_Jacobian(blst_p1 *out, const blst_p1xyzz *in);   /* ec_ops.h:771-777 */
void blst_p2xyzz_to_Jacobian(blst_p2 *out, const blst_p2xyzz *in);
void blst_p1_to_xyzz(blst_p1xyzz *out, blst_p1 *in);                /* ec_ops.h:779-785 */
void blst_p2_to_xyzz(blst_p2xyzz *out, blst_p2 *in);
void blst_p1_prefetch_CHES(const blst_p1xyzz buckets[], size_t booth_idx);  /* no-op hint */
void blst_p2_prefetch_CHES(const blst_p2xyzz buckets[], size_t booth_idx);
void blst_p1_bucket_CHES(blst_p1xyzz buckets[], int booth_idx, const blst_p1_affine *p,
                         unsigned char booth_sign);                  /* multi_scalar.c:358-361 */
void blst_p2_bucket_CHES(blst_p2xyzz buckets[], int booth_idx, const blst_p2_affine *p, unsigned char booth_sign);
/* sum_i bucket_set_ascend[i] * buckets[i] (multi_scalar.c:301-321); any non-negative
 * weights are accepted (d_max is not needed by the GPU reduction) */
void blst_p1_integrate_buckets_accumulation_d_CHES(blst_p1 *out, blst_p1xyzz buckets[], int bucket_set_ascend[],
                                                   size_t bucket_set_size, int d_max);
void blst_p2_integrate_buckets_accumulation_d_CHES(blst_p2 *out, blst_p2xyzz buckets[], int bucket_set_ascend[],
                                                   size_t bucket_set_size, int d_max);
/* integral scalar conversion (multi_scalar.c:748-775): standard q-ary digits in
 * nh_scalars[] (carry written into the next slot) -> bucket values, signs, table pointers */
void blst_p1_construct_nh_scalars_nh_points(int nh_scalars[], unsigned char booth_signs[],
                                            blst_p1_affine *nh_points_ptr[], const size_t npoints,
                                            blst_p1_affine precomputation_points_list_3nh[],
                                            const digit_decomposition digit_conversion_hash_table[]);
void blst_p2_construct_nh_scalars_nh_points(int nh_scalars[], unsigned char booth_signs[],
                                            blst_p2_affine *nh_points_ptr[], const size_t npoints,
                                            blst_p2_affine precomputation_points_list_3nh[],
                                            const digit_decomposition digit_conversion_hash_table[]);
/* CHES accumulation + d-reduction (multi_scalar.c:421-463, 643-655) */
void blst_p1_tile_pippenger_d_CHES(blst_p1 *ret, const blst_p1_affine *const points[], size_t npoints,
                                   const int scalars[], const unsigned char booth_signs[], blst_p1xyzz buckets[],
                                   int bucket_set_ascend[], int bucket_value_to_its_index[], size_t bucket_set_size,
                                   int d_max);
void blst_p2_tile_pippenger_d_CHES(blst_p2 *ret, const blst_p2_affine *const points[], size_t npoints,
                                   const int scalars[], const unsigned char booth_signs[], blst_p2xyzz buckets[],
                                   int bucket_set_ascend[], int bucket_value_to_its_index[], size_t bucket_set_size,
                                   int d_max);
/* buckets indexed by bucket value (multi_scalar.c:466-503); values outside the set weigh 0 */
void blst_p1_tile_pippenger_d_CHES_noindexhash(blst_p1 *ret, const blst_p1_affine *const points[], size_t npoints,
                                               const int scalars[], const unsigned char booth_signs[],
                                               blst_p1xyzz buckets[], int bucket_set_ascend[], size_t bucket_set_size,
                                               int d_max);
void blst_p2_tile_pippenger_d_CHES_noindexhash(blst_p2 *ret, const blst_p2_affine *const points[], size_t npoints,
                                               const int scalars[], const unsigned char booth_signs[],
                                               blst_p2xyzz buckets[], int bucket_set_ascend[], size_t bucket_set_size,
                                               int d_max);
/* standard q-ary digits in, digit-hash lookup + carry inside (multi_scalar.c:671-744);
 * scalars[] is updated with the carries as the reference does (needs one slot of padding) */
void blst_p1_tile_pippenger_CHES_prefetch_2step_ahead_input_std_scalar(
    blst_p1 *ret, const blst_p1_affine precomputation_points_list_3nh[], size_t npoints, int scalars[],
    digit_decomposition digit_conversion_hash_table[], blst_p1xyzz buckets[], int bucket_set_ascend[],
    int bucket_value_to_its_index[], size_t bucket_set_size, int d_max);
void blst_p2_tile_pippenger_CHES_prefetch_2step_ahead_input_std_scalar(
    blst_p2 *ret, const blst_p2_affine precomputation_points_list_3nh[], size_t npoints, int scalars[],
    digit_decomposition digit_conversion_hash_table[], blst_p2xyzz buckets[], int bucket_set_ascend[],
    int bucket_value_to_its_index[], size_t bucket_set_size, int d_max);
/* BGMW95 accumulation + running-sum reduction (multi_scalar.c:506-547); |digits| <= q/2 */
void blst_p1_tile_pippenger_BGMW95(blst_p1 *ret, const blst_p1_affine *const points[], size_t npoints,
                                   const int scalars[], const unsigned char booth_signs[], blst_p1xyzz buckets[],
                                   size_t q_exponent);
void blst_p2_tile_pippenger_BGMW95(blst_p2 *ret, const blst_p2_affine *const points[], size_t npoints,
                                   const int scalars[], const unsigned char booth_signs[], blst_p2xyzz buckets[],
                                   size_t q_exponent);

/* ---- sum of affine points (replaces ref src/bulk_addition.c:145-164, blst.h:224-225) ----
 * ret = sum of npoints affine points (all-zero = infinity).  Pointer rule of
 * bulk_addition.c:155: a NULL entry means "the point right after the previous one"
 * ({ptr, NULL} = one flat array).  On the GPU: entries spread over buckets of
 * weight 1, one lane per bucket, then the bucket reduction. */
void blst_p1s_add(blst_p1 *ret, const blst_p1_affine *const points[], size_t npoints);
void blst_p2s_add(blst_p2 *ret, const blst_p2_affine *const points[], size_t npoints);

/* ---- fixed-window MSM with a precomputed table (replaces ref src/multi_scalar.c:63-261,
 * blst.h:228-236 and :367-375; used by the C++ binding's P1_Affines / P2_Affines,
 * ref bindings/blst.hpp:362-430) ----
 * Same semantics and table layout as blst: table row i holds the canonical affine
 * multiples (k+1) P_i, k < 2^(wbits-1), wbits in [2, 14]; precompute may be called
 * with the points stored inside the output table (blst.hpp:383-393); the pointer
 * rules of blst apply to points[] and scalars[] (stride (nbits+7)/8).  On the GPU:
 * precompute builds every row by repeated mixed additions and one batch inversion
 * per point; mult sums the Booth-digit gathers of each window in parallel and
 * combines the window totals on the host.  The table is uploaded on every mult
 * call (the msm_wbits_ctx_* API below keeps it resident).  scratch is not used. */
size_t blst_p1s_mult_wbits_precompute_sizeof(size_t wbits, size_t npoints);
void blst_p1s_mult_wbits_precompute(blst_p1_affine table[], size_t wbits, const blst_p1_affine *const points[],
                                    size_t npoints);
size_t blst_p1s_mult_wbits_scratch_sizeof(size_t npoints);
void blst_p1s_mult_wbits(blst_p1 *ret, const blst_p1_affine table[], size_t wbits, size_t npoints,
                         const byte *const scalars[], size_t nbits, limb_t *scratch);
size_t blst_p2s_mult_wbits_precompute_sizeof(size_t wbits, size_t npoints);
void blst_p2s_mult_wbits_precompute(blst_p2_affine table[], size_t wbits, const blst_p2_affine *const points[],
                                    size_t npoints);
size_t blst_p2s_mult_wbits_scratch_sizeof(size_t npoints);
void blst_p2s_mult_wbits(blst_p2 *ret, const blst_p2_affine table[], size_t wbits, size_t npoints,
                         const byte *const scalars[], size_t nbits, limb_t *scratch);

/* ---- extension API: device-resident contexts (points uploaded once) ---- */
enum {
  MSM_OK = 0,
  MSM_E_ARG = -1,      /* bad argument */
  MSM_E_HIP = -2,      /* HIP runtime failure (message in msm_last_error) */
  MSM_E_NODEV = -3,    /* no gfx950 device visible */
  MSM_E_STATE = -4     /* context not ready (e.g. tables not built) */
};
typedef struct msm_ctx msm_ctx;
const char *msm_last_error(void);
/* void blst-named entry points on failure: 1 = print + abort (default), 0 = return
 * with the all-zero result and raise msm_error_pending(); returns the previous mode */
int msm_set_abort_on_error(int on);
/* nonzero if a blst-named call of this thread failed since the last query (clears it) */
int msm_error_pending(void);
int msm_device_count(void);
/* The VALU ceilings of `device`, measured now by register-resident kernels
 * (extension, no reference counterpart; bench.py prices its roofline with them
 * in the same run): out = {v_mad_u64_u32 lane-ops/s, Fp-mul/s, G1 xyzz madd/s
 * (the accumulation's loop body, rows in cache), device ms spent} */
int msm_valu_probe(int device, double out[4]);
/* Device self-test of the two Montgomery column forms (extension): every lane t of
 * `lanes` reads 8 field elements a0..a7 (internal form: 14 words of 28 bits, each
 * normalized and < 2p) and writes 11: a0 a1, a0^2, a0 a1 + a2 a3, the xyzz point
 * (a0..a3) plus the affine row (a4, a5) (negated on odd lanes), and the xyzz point
 * (a0..a3) plus the xyzz point (a4..a7).  form 0: split columns, 1: single chain. */
int msm_fp_form_ops(int device, int form, const uint32_t *in, size_t lanes, uint32_t *out);
/* Engines behind the blst-named entry points (no caller context: ref
 * multi_scalar.c:581-607) live in a process-wide pool per (device, kind,
 * window): a call leases one, a concurrent call creates another, and a returned
 * engine stays cached while the idle engines of its kind on its device hold at
 * most the cache limit of device memory (default 8 GiB); device memory is thus
 * bounded by the peak number of concurrent calls, not by the number of calling
 * threads.  release: frees every idle engine now.  stats: out[0] engines alive
 * (leased + idle), out[1] idle, out[2] device bytes held by idle engines.
 * set_limit returns the previous limit. */
void msm_release_engine_cache(void);
void msm_engine_cache_stats(size_t out[3]);
size_t msm_set_engine_cache_limit(size_t bytes);
/* Registered host tables (extension for the pointer-array tiles above).  The
 * reference driver hands the SAME host table to every CHES tile call, as one
 * pointer per entry into PRECOMPUTATION_POINTS_LIST_3nh (ref main_p1.cpp:233-236,
 * :279-282; 3 n h rows, built once by init_pippenger_CHES_q_over_5 :128-178).
 * Registering those rows once uploads them to the current device; afterwards a
 * tile call (blst_p{1,2}_tile_pippenger_d_CHES, _noindexhash, _BGMW95) whose
 * pointers all lie on row boundaries inside one registered table sends 4-B row
 * indices instead of gathering and uploading every 96/192-B row (1.2 GB per
 * G1 2^20 call).  Any pointer outside the table falls back to the gather.  A
 * point array registered the same way serves the plain drop-in: a flat
 * {ptr, NULL} blst_p{1,2}s_mult_pippenger / _tile_pippenger call whose npoints
 * points lie inside one registered table reads their device copy instead of
 * uploading 96/192 B per point (ref multi_scalar.c:549-607; callers that
 * multiply one SRS many times).  The
 * caller must not modify or free the rows while they are registered (as with
 * hipHostRegister).  Guard: up to 1024 rows at even strides (first and last
 * included) are sampled at registration; a call whose rows include a sample
 * that no longer matches the host memory re-uploads the table first, so a
 * reused or rewritten buffer is caught (an edit of one unsampled row is not).  group 1 (G1, blst_p1_affine rows) or 2 (G2); registering
 * an already registered base replaces it.  Returns MSM_OK or an error code. */
int msm_register_host_table(int group, const void *rows_affine, size_t nrows);
int msm_unregister_host_table(const void *rows_affine);
/* group 1 (G1) or 2 (G2); points in blst affine layout, host or device memory */
int msm_ctx_create(msm_ctx **ctx, int group, int device, int window_bits);
int msm_ctx_set_points(msm_ctx *ctx, const void *points_affine, size_t npoints, int points_on_device,
                       void *hip_stream);
/* scalars: npoints byte strings with the given stride (32 for blst_scalar arrays),
 * on host or device; ret: blst_p1 / blst_p2 Jacobian (host memory) */
int msm_ctx_mult(msm_ctx *ctx, void *ret, const byte *scalars, size_t stride, size_t nbits, int scalars_on_device,
                 void *hip_stream);
/* `count` MSMs over the context's points in one pipelined call (extension: the
 * shape of a prover committing many polynomials to one SRS; ref
 * main_p1.cpp:470-476 runs 5 scalar arrays back to back): scalar set k at
 * scalars + k * set_stride, each npoints strings of `stride` bytes; rets: count
 * Jacobians.  scalars_on_device = 0: the sets are uploaded first.  Results equal
 * `count` msm_ctx_mult calls. */
int msm_ctx_mult_batch(msm_ctx *ctx, void *rets, const byte *scalars, size_t stride, size_t set_stride,
                       size_t nbits, size_t count, int scalars_on_device, void *hip_stream);
int msm_ctx_set_profiling(msm_ctx *ctx, int on);
/* per-phase device ms of the last msm_ctx_mult (profiling on):
 * [digits, sort, accumulate, reduce, finalize, total] */
int msm_ctx_phase_times(const msm_ctx *ctx, float out[6]);
void msm_ctx_destroy(msm_ctx *ctx);

/* ---- CHES "nh + q/5" bucket-set method, device-resident precomputed table ----
 * Replaces the driver-level CHES path of ref main_p1.cpp: init_pippenger_CHES_q_over_5
 * (:128-178: bucket set, digit hash, table T[3(i h + j) + m - 1] = m q^j P_i) and
 * pippenger_variant_q_over_5_CHES (:192-246: MB digit conversion, accumulation
 * blst_p1_tile_pippenger_d_CHES, reduction :301-321).  The table is built on
 * the GPU (or uploaded) once; each mult takes n 32-byte scalars.  The result is
 * the true sum_i s_i P_i (the reference's last-element guard defect,
 * multi_scalar.c:461, is not reproduced; scalars >= r are reduced mod r where
 * the reference requires s < r). */
typedef struct msm_ches_ctx msm_ches_ctx;
/* the configuration of ref ches_config_files/config_file_n_exp_<n_exp>[_beta].h:
 * out = {n_exp, beta, q_exp, h, a_h, d_max, b_size, q_exp_bgmw, h_bgmw} */
int msm_ches_params(int n_exp, int beta, int out[9]);
int msm_ches_ctx_create(msm_ches_ctx **ctx, int group, int device, int n_exp, int beta);
/* explicit parameters (same 9-int layout; b_size 0 = not checked) */
int msm_ches_ctx_create_params(msm_ches_ctx **ctx, int group, int device, const int params[9]);
/* One MSM over several devices from one process (the reference is
 * single-device, its Go binding splits points x windows over CPU threads,
 * bindings/go/blst.go:2064-2197).  The points are split into ndev contiguous
 * balanced shards, shard g on devices[g] with its own rows of the reference
 * table (the rows of point i are contiguous in main_p1.cpp:155-172's layout, so
 * set/get/save/load_table keep that layout); each mult runs every shard
 * concurrently and folds the 144/288-B partials exactly on the host.  n_exp /
 * beta select the configuration of ONE SHARD (e.g. 2^21 points over 8 devices:
 * n_exp = 18).  Devices may repeat (several shards on one device).  Points,
 * table rows and scalars must be in host memory when ndev > 1. */
int msm_ches_ctx_create_multi(msm_ches_ctx **ctx, int group, const int *devices, int ndev, int n_exp, int beta);
int msm_ches_ctx_shards(const msm_ches_ctx *ctx);
/* 1 if this context's batches exchange their partials over RCCL (opt-in:
 * MSM_MULTI_RCCL=1 with shards on distinct devices; round 6 made it opt-in
 * until a run on several devices has checked it), 0 if each shard is read back */
int msm_ches_ctx_rccl_exchange(const msm_ches_ctx *ctx);
/* base points P_i (blst affine) -> T built on the GPU */
int msm_ches_ctx_build_table(msm_ches_ctx *ctx, const void *points_affine, size_t npoints, int on_device,
                             void *hip_stream);
/* a precomputed T (blst affine, 3 * npoints * h entries, main_p1.cpp:155-172 order) */
int msm_ches_ctx_set_table(msm_ches_ctx *ctx, const void *table_affine, size_t npoints, int on_device,
                           void *hip_stream);
/* T[first, first + count) in blst affine layout, to host memory */
int msm_ches_ctx_get_table(msm_ches_ctx *ctx, void *out_affine, size_t first, size_t count);
/* scalars: npoints 32-byte LE strings with the given stride (>= 32), host or device */
int msm_ches_ctx_mult(msm_ches_ctx *ctx, void *ret, const byte *scalars, size_t stride, int scalars_on_device,
                      void *hip_stream);
/* count MSMs over the same points: scalar set k (npoints strings of `stride` bytes)
 * at scalars + k * set_stride; rets: count Jacobians.  Pipelined on the device:
 * MSM k's latency-bound bucket-reduction tail runs on a second stream beside
 * MSM k+1's digit conversion, sort and accumulation (the batched-MSM shape of a
 * prover committing many polynomials to one SRS).  Results equal count calls
 * of msm_ches_ctx_mult.  Host scalars (scalars_on_device = 0) are copied set by
 * set inside the pipeline, each copy overlapping earlier MSMs' accumulations;
 * pass page-locked memory (hipHostMalloc / hipHostRegister) for the copies to
 * be asynchronous. */
int msm_ches_ctx_mult_batch(msm_ches_ctx *ctx, void *rets, const byte *scalars, size_t stride, size_t set_stride,
                            size_t count, int scalars_on_device, void *hip_stream);
/* table file cache (the reference rebuilds its tables on every run, main_p1.cpp:128-178):
 * 64-byte header + the rows in blst affine layout; load checks group/method/q/h */
int msm_ches_ctx_save_table(msm_ches_ctx *ctx, const char *path);
int msm_ches_ctx_load_table(msm_ches_ctx *ctx, const char *path);
int msm_ches_ctx_set_profiling(msm_ches_ctx *ctx, int on);
int msm_ches_ctx_phase_times(const msm_ches_ctx *ctx, float out[6]);
size_t msm_ches_ctx_bucket_count(const msm_ches_ctx *ctx);
/* accumulation lanes msm_ches_ctx_mult_batch runs (first shard's engine): 1 when
 * one accumulation fills the chip >= 3 wave-slot rounds deep, else 2-3 MSMs
 * accumulate side by side (MSM_BATCH_LANES overrides); 0 on a NULL ctx */
int msm_ches_ctx_batch_lanes(const msm_ches_ctx *ctx);
/* diagnostic (single-device contexts): digits + sort of nsets scalar sets in
 * DEVICE memory (set_stride bytes apart, 32-byte scalars), then the mean ms of
 * reps launches accumulating all nsets sets in one grid, alone on the stream */
int msm_ches_ctx_time_accumulation(msm_ches_ctx *ctx, const byte *scalars_dev, size_t set_stride, int nsets, int reps,
                                   float *ms_per_launch);
void msm_ches_ctx_destroy(msm_ches_ctx *ctx);

/* ---- BGMW95 fixed-base method, device-resident precomputed table ----
 * Replaces ref main_p1.cpp:94-122 init_pippenger_BGMW95 (table T[i h + j] = q^j P_i)
 * and :294-398 pippenger_variant_BGMW95 (signed radix-q digits in (-q/2, q/2],
 * r - s for large top digits, one set of q/2 buckets, tile
 * blst_p1_tile_pippenger_BGMW95 multi_scalar.c:506-547 + integrate :281-297).
 * q = 2^q_exp with q_exp * h >= 255; the reference's per-n choice is
 * msm_ches_params(...)[7..8] (EXPONENT_OF_q_BGMW95, h_BGMW95). */
typedef struct msm_bgmw_ctx msm_bgmw_ctx;
int msm_bgmw_ctx_create(msm_bgmw_ctx **ctx, int group, int device, int q_exp, int h);
int msm_bgmw_ctx_build_table(msm_bgmw_ctx *ctx, const void *points_affine, size_t npoints, int on_device,
                             void *hip_stream);
/* a precomputed T (blst affine, npoints * h entries, main_p1.cpp:109-119 order) */
int msm_bgmw_ctx_set_table(msm_bgmw_ctx *ctx, const void *table_affine, size_t npoints, int on_device,
                           void *hip_stream);
int msm_bgmw_ctx_get_table(msm_bgmw_ctx *ctx, void *out_affine, size_t first, size_t count);
int msm_bgmw_ctx_mult(msm_bgmw_ctx *ctx, void *ret, const byte *scalars, size_t stride, int scalars_on_device,
                      void *hip_stream);
int msm_bgmw_ctx_save_table(msm_bgmw_ctx *ctx, const char *path);
int msm_bgmw_ctx_load_table(msm_bgmw_ctx *ctx, const char *path);
int msm_bgmw_ctx_set_profiling(msm_bgmw_ctx *ctx, int on);
int msm_bgmw_ctx_phase_times(const msm_bgmw_ctx *ctx, float out[6]);
size_t msm_bgmw_ctx_bucket_count(const msm_bgmw_ctx *ctx);
void msm_bgmw_ctx_destroy(msm_bgmw_ctx *ctx);

/* ---- fixed-window (wbits) MSM with the table resident in HBM ---- */
typedef struct msm_wbits_ctx msm_wbits_ctx;
int msm_wbits_ctx_create(msm_wbits_ctx **ctx, int group, int device, int wbits);
/* base points (blst affine, host or device) -> the table, built on the GPU */
int msm_wbits_ctx_precompute(msm_wbits_ctx *ctx, const void *points_affine, size_t npoints, int on_device,
                             void *hip_stream);
/* a table in the reference layout (npoints << (wbits-1) blst affine rows), host or device */
int msm_wbits_ctx_set_table(msm_wbits_ctx *ctx, const void *table_affine, size_t npoints, int on_device,
                            void *hip_stream);
int msm_wbits_ctx_get_table(msm_wbits_ctx *ctx, void *out_affine, size_t first, size_t count);
/* scalars: npoints LE strings of `stride` bytes (>= (nbits+7)/8), host or device; low nbits bits */
int msm_wbits_ctx_mult(msm_wbits_ctx *ctx, void *ret, const byte *scalars, size_t stride, size_t nbits,
                       int scalars_on_device, void *hip_stream);
size_t msm_wbits_ctx_table_rows(const msm_wbits_ctx *ctx);
void msm_wbits_ctx_destroy(msm_wbits_ctx *ctx);

/* ---- bulk Jacobian -> affine (replaces ref src/multi_scalar.c:17-62, blst_p{1,2}s_to_affine;
 * blst.h:222-223, :362; what blst.hpp:389,406,438 calls) ----
 * dst[i] = the canonical affine form of point i (fully reduced, blst Montgomery
 * layout; byte-identical to the reference's for finite points).  Named msm_, not
 * blst_: the reference's own blst_p{1,2}s_to_affine stays global in a caller that
 * links both libraries; a caller forwards in one line.
 * msm_p{1,2}s_to_affine: pointer rule of multi_scalar.c:30 (a NULL entry means "the
 * point right after the previous one", and the array is not read past it: {ptr, NULL}
 * is one flat array); points and dst in host memory; runs on the current device.
 * msm_points_to_affine: flat arrays, each side in host or device memory (device
 * pointers 8-byte aligned), on HIP device `device`.
 * On the GPU: one batch inversion over each chunk of points (default 2^18,
 * MSM_TO_AFFINE_CHUNK=<points> overrides, read at each call), as a tree of products
 * of 8 (k_ta_up / k_ta_leaf / k_ta_down, csrc/to_affine.hip), about 9.7 field products
 * per point; device memory is bounded by the chunk, not by npoints; host memory goes
 * through two pinned staging buffers per direction, copies overlapping the kernels.
 * Difference, toward the exact result: a point with Z = 0 is infinity whatever its X
 * and Y hold; its output is the all-zero affine point and no other output is
 * affected.  (The reference multiplies Z = 0 into the product shared by a stride of
 * 1536 / 768 points and corrupts all of them, its own comment at multi_scalar.c:14-16;
 * the same defect the wbits "inf" cases record.)
 * npoints == 0: MSM_OK, nothing touched.  MSM_E_ARG, before any device work: NULL dst
 * or source with npoints > 0, group other than 1 or 2, overlapping host ranges.
 * MSM_E_NODEV: no such device.  MSM_E_HIP: a HIP failure (msm_last_error()); a host
 * dst is then zero-filled, never half written; a device dst is unspecified.
 * Streams: the call first waits for the work queued earlier on hip_stream (device
 * sources are read by kernels ordered on it; for a host source the stream is
 * drained).  With a device dst the work is ordered on hip_stream and the call may
 * return before it finishes (hip_stream NULL: it has finished); with a host dst the
 * call returns with the data there.  Thread-safe per call: each call leases an
 * engine from the pool keyed by (device, group), released by
 * msm_release_engine_cache() and counted by msm_engine_cache_stats(). */
int msm_p1s_to_affine(blst_p1_affine dst[], const blst_p1 *const points[], size_t npoints);
int msm_p2s_to_affine(blst_p2_affine dst[], const blst_p2 *const points[], size_t npoints);
int msm_points_to_affine(int group, int device, void *dst_affine, const void *src_jacobian, size_t npoints,
                         int src_on_device, int dst_on_device, void *hip_stream);
/* diagnostic: number of product levels (k_ta_up launches) the plan uses above the
 * points of one chunk for this n */
int msm_to_affine_levels(size_t npoints);

/* ---- bulk point decoding (replaces the reference's one-point blst_p{1,2}_uncompress,
 * blst_p{1,2}_deserialize and blst_p{1,2}_affine_in_g{1,2}: ref src/e1.c:236-351,
 * src/e2.c:279-410, src/map_to_g1.c:531-559, src/map_to_g2.c:403-443) ----
 * src: npoints ZCash-encoded entries of 48 G bytes (MSM_ENC_COMPRESSED) or 96 G bytes
 * (MSM_ENC_SERIALIZED), G = group.  Entry i is decoded as the reference decodes it: an
 * entry of a serialized array whose compressed bit is set has its first 48 G bytes
 * decoded as a compressed point; infinity is c0 00.. / 40 00...
 * status[i] is the reference's return code: 0 success, 1 bad encoding, 2 not on the
 * curve, 3 not in the group (the reference itself: only G1 x = 0).  With
 * MSM_DECODE_CHECK_GROUP an entry that would be 0 and lies outside the prime-order
 * subgroup (blst_p{1,2}_affine_in_g{1,2} false) gets 3; infinity passes.
 * dst[i] of a status-0 entry is the canonical affine point in blst Montgomery layout,
 * byte-identical to the reference's (infinity: all zero).  Difference, toward safety:
 * dst[i] of every entry with a non-zero status is the all-zero point (the reference
 * leaves its output untouched, or for G1 x = 0 written), so a failed point can enter
 * an MSM only as the identity.
 * status and nbad are host memory and may be NULL; nbad receives the number of
 * non-zero statuses.  src and dst each in host or device memory (device src 4-byte,
 * device dst 8-byte aligned), on HIP device `device`.
 * npoints == 0: MSM_OK, nothing touched.  MSM_E_ARG, before any device work: NULL dst
 * or src with npoints > 0, group other than 1 or 2, unknown encoding, unknown flag
 * bits, overlapping host ranges.  MSM_E_NODEV: no such device.  MSM_E_HIP: a HIP
 * failure; a host dst is then zero-filled and status, if given, filled with 1.
 * Streams as msm_points_to_affine; in addition a call with status or nbad returns
 * only when they are written.  On the GPU: csrc/decode.hip, chunks of at most 2^18
 * entries (MSM_DECODE_CHUNK=<entries> overrides, read at each call), host memory
 * through two pinned staging buffers per direction.  Thread-safe per call (an engine
 * pool keyed by (device, group), counted by msm_engine_cache_stats(), freed by
 * msm_release_engine_cache()). */
enum { MSM_ENC_COMPRESSED = 0, MSM_ENC_SERIALIZED = 1 }; /* stride 48 G / 96 G bytes per entry */
enum { MSM_DECODE_CHECK_GROUP = 1 };                     /* flags */
int msm_points_decode(int group, int device, void *dst_affine, uint8_t *status, size_t *nbad, const void *src,
                      size_t npoints, int encoding, int flags, int src_on_device, int dst_on_device,
                      void *hip_stream);
/* decode into a device buffer the context owns, then msm_ctx_set_points(.., on device).
 * Any non-zero status: the context keeps its previous points, MSM_E_ARG is returned,
 * *first_bad (may be NULL) is the lowest failing index and msm_last_error() names
 * index and status. */
int msm_ctx_set_points_encoded(msm_ctx *ctx, const void *src, size_t npoints, int encoding, int flags,
                               int src_on_device, size_t *first_bad, void *hip_stream);

/* ---- bulk scalar multiplication (replaces a loop over the reference's one-point
 * blst_p{1,2}_mult / blst_p{1,2}_unchecked_mult: ref src/e1.c:505-533, src/e2.c,
 * src/ec_mult.h) ----
 * dst[i] = [k_i] P_i as a canonical affine point in blst Montgomery layout (infinity:
 * all zero), for i < npoints.  P_i: affine point i of points_affine (all zero:
 * infinity, which gives infinity); with MSM_MULT_ONE_POINT points_affine holds ONE
 * point, used for every scalar (fixed base).  k_i: the integer in the low nbits bits
 * of the little-endian scalar at scalars + i scalar_stride, 0 <= nbits <= 256,
 * (nbits + 7) / 8 <= scalar_stride <= 2^20.  Bits at and above nbits in the last byte are
 * ignored (masked), and no byte beyond (nbits + 7) / 8 of a scalar is read.
 * nbits == 0: every output is infinity.
 * The result is the exact [k_i] P_i for every point of the curve, in the prime-order
 * subgroup or not: the contract of blst_p{1,2}_unchecked_mult, which coincides with
 * blst_p{1,2}_mult on subgroup points.  (No endomorphism split of the scalar is used;
 * it is only valid inside the subgroup.)
 * points and scalars are both in host memory or both in device memory
 * (src_on_device; device points 8-byte aligned, scalars unaligned); dst in host or
 * device memory (8-byte aligned), on HIP device `device`.
 * npoints == 0: MSM_OK, nothing touched.  MSM_E_ARG, before any device work: a NULL
 * pointer with npoints > 0, group other than 1 or 2, nbits > 256, a scalar_stride
 * shorter than (nbits + 7) / 8, unknown flag bits, host sources overlapping a host
 * dst.  MSM_E_NODEV: no such device.  MSM_E_HIP: a HIP failure; a host dst is then
 * zero-filled.  Streams as msm_points_to_affine.  On the GPU: csrc/points_mult.hip, a
 * ladder over signed 4-bit windows on a per-point table of 8 affine rows kept in
 * device memory for one chunk of at most 2^18 points (MSM_POINTS_MULT_CHUNK=<points>
 * overrides, read at each call), host memory through two pinned staging buffers per
 * direction.  Thread-safe per call (an engine pool keyed by (device, group), counted
 * by msm_engine_cache_stats(), freed by msm_release_engine_cache()). */
#define MSM_MULT_ONE_POINT 1 /* points_affine holds ONE point, used for every scalar (fixed base) */
int msm_points_mult(int group, int device, void *dst_affine, const void *points_affine, const byte *scalars,
                    size_t npoints, size_t nbits, size_t scalar_stride, int flags, int src_on_device,
                    int dst_on_device, void *hip_stream);

/* ---- segmented sums and MSMs over many point sets (replaces a host loop over the
 * reference's blst_p{1,2}s_mult_pippenger / blst_p{1,2}s_add, one call per point set:
 * ref src/multi_scalar.c:581-607, src/bulk_addition.c:145-164) ----
 * With o = offsets and k = nsegments:
 *   dst[j] = sum over o[j] <= i < o[j + 1] of [k_i] P_i        for j < k,
 * each a canonical affine point in blst Montgomery layout (infinity: all zero).
 * offsets is always a HOST array of k + 1 values, non-decreasing.  o[k] points and
 * scalars are read, indexed from 0; those below o[0] are ignored.  An empty segment
 * gives infinity.  P_i: affine point i of points_affine; an all-zero point is infinity
 * and contributes nothing.  scalars == NULL means plain sums, every k_i = 1 (nbits and
 * scalar_stride are then ignored).  Otherwise k_i, nbits and scalar_stride are exactly
 * as in msm_points_mult: the low nbits bits of the little-endian scalar at scalars +
 * i scalar_stride, 0 <= nbits <= 256, (nbits + 7) / 8 <= scalar_stride <= 2^20, stray
 * bits in the last byte masked, no byte beyond (nbits + 7) / 8 of a scalar read;
 * nbits == 0 makes every result infinity.
 * The result is exact for every point of the curve, in the prime-order subgroup or not
 * (the contract of msm_points_mult; no endomorphism split is used).
 * points and scalars are both in host memory or both in device memory (src_on_device;
 * device points 8-byte aligned, scalars unaligned); dst in host or device memory
 * (8-byte aligned), on HIP device `device`.  flags must be 0.
 * nsegments == 0: MSM_OK, nothing touched.  MSM_E_ARG, before any device work: NULL
 * dst / points / offsets with nsegments > 0, a decreasing offset, group other than 1
 * or 2, nbits > 256, a scalar_stride shorter than (nbits + 7) / 8, non-zero flags, a
 * host dst overlapping a host source.  MSM_E_NODEV: no such device.  MSM_E_HIP: a HIP
 * failure; a host dst is then zero-filled.  Streams as msm_points_to_affine.
 * On the GPU: csrc/point_segments.hip.  The host cuts the points into pieces of at
 * most L consecutive points of one segment; one lane (G2: a lane pair) runs a Straus
 * ladder over signed 4-bit windows on the per-point table of msm_points_mult, with
 * the four doublings of a window shared by the points of its piece (plain sums: one
 * pass of mixed additions, no table); the partial sums of a segment are merged by a
 * pairwise tree and the k sums normalised by the inversion tree of
 * msm_points_to_affine.  L grows with the number of points until the pieces would no
 * longer fill the chip, 1 <= L <= 64 (MSM_POINTS_SEGMENTS_PIECE=<points> overrides);
 * chunks are sized by the device memory they allocate, about 3 GiB
 * (MSM_POINTS_SEGMENTS_CHUNK=<points> overrides; both read at each call); a segment
 * may span chunks.  Host memory goes through two pinned staging buffers per direction.
 * There is no bucket method inside a segment: a single very long segment is better
 * served by a context (msm_ctx_mult and its kin).  For encoded output chain
 * msm_points_encode on a device dst.  Thread-safe per call (an engine pool keyed by
 * (device, group), counted by msm_engine_cache_stats(), freed by
 * msm_release_engine_cache()). */
int msm_points_msm_segments(int group, int device, void *dst_affine, const void *points_affine, const byte *scalars,
                            const size_t *offsets, size_t nsegments, size_t nbits, size_t scalar_stride, int flags,
                            int src_on_device, int dst_on_device, void *hip_stream);
/* host only, no device work: the piece length L a call over npoints points would use */
size_t msm_segments_piece(int group, size_t npoints);
/* host only, no device work: the pieces that `piece` (> 0) cuts offsets into, in
 * order.  *npieces receives their number; the first `capacity` of them are written to
 * start[] (first point), count[] (points, <= piece) and segment[] (each may be NULL).
 * MSM_E_ARG: NULL npieces / offsets, piece == 0, a decreasing offset. */
int msm_segments_plan(const size_t *offsets, size_t nsegments, size_t piece, size_t *npieces, size_t *start,
                      size_t *count, size_t *segment, size_t capacity);

/* ---- bulk point encoding (replaces a loop over the reference's one-point
 * blst_p{1,2}_affine_compress / _affine_serialize / _compress / _serialize: ref
 * src/e1.c:139-234 and the src/e2.c twins) ----
 * src: npoints flat blst affine points (96 G bytes, MSM_SRC_AFFINE) or blst Jacobians
 * (144 G bytes, MSM_SRC_JACOBIAN), G = group.  dst: npoints ZCash entries of 48 G bytes
 * (MSM_ENC_COMPRESSED) or 96 G bytes (MSM_ENC_SERIALIZED).  Entry i is byte-identical
 * to the reference call for its source form and encoding.  Nothing is validated and
 * there is no status: whatever coordinates are given are encoded, on the curve or not.
 * Affine infinity is the all-zero point (X zero with Y non-zero is a finite entry), a
 * Jacobian is infinity when Z is zero whatever X and Y hold; infinity encodes as
 * c0 00.. / 40 00...  Finite points: canonical big-endian coordinates (G2: imaginary
 * part first); compressed entries carry 0x80 and, when y is larger than -y (G2: by the
 * imaginary part unless it is zero), 0x20.  Affine limbs in [p, 2^384) encode their
 * value mod p (as the reference, whose sign rule counts y limbs that are a non-zero
 * multiple of p as p itself: flag set, bytes zero); non-canonical Jacobian coordinates
 * are unspecified.
 * src and dst each in host or device memory (device src 8-byte, device dst 4-byte
 * aligned), on HIP device `device`.  flags must be 0.
 * npoints == 0: MSM_OK, nothing touched.  MSM_E_ARG, before any device work: a NULL
 * pointer with npoints > 0, group other than 1 or 2, unknown source form, unknown
 * encoding, non-zero flags, overlapping host ranges.  MSM_E_NODEV: no such device.
 * MSM_E_HIP: a HIP failure; a host dst is then zero-filled.  Streams as
 * msm_points_to_affine.  On the GPU: csrc/encode.hip, 2 G field products per affine
 * point; Jacobians go through the inversion tree of msm_points_to_affine, whose last
 * kernel writes the entries (no affine array in between); chunks of at most 2^18
 * points (MSM_ENCODE_CHUNK=<points> overrides, read at each call), host memory through
 * two pinned staging buffers per direction.  Thread-safe per call (an engine pool
 * keyed by (device, group), counted by msm_engine_cache_stats(), freed by
 * msm_release_engine_cache()). */
enum { MSM_SRC_AFFINE = 0, MSM_SRC_JACOBIAN = 1 };
int msm_points_encode(int group, int device, void *dst, const void *src, size_t npoints, int src_form, int encoding,
                      int flags, int src_on_device, int dst_on_device, void *hip_stream);

/* ---- bulk hash-to-curve (replaces a loop over the reference's one-message
 * blst_hash_to_g{1,2} / blst_encode_to_g{1,2} / blst_map_to_g{1,2}: ref
 * src/map_to_g1.c:285-453, src/map_to_g2.c:173-401, src/hash_to_field.c:51-154;
 * RFC 9380, expand_message_xmd over SHA-256, simplified SWU, 11- / 3-isogeny) ----
 * msm_points_map: u holds npoints * count field elements in blst's Montgomery layout
 * (48 G bytes each, blst_fp / blst_fp2), canonical; nothing is validated.  count is 1
 * or 2.  dst[i] is the affine form of blst_map_to_g{1,2}(u[i count], count == 2 ?
 * u[i count + 1] : NULL), byte for byte; infinity is the all-zero point.
 * msm_hash_to_field: message i is msgs[offsets[i] .. offsets[i + 1]), offsets a HOST
 * array of npoints + 1 non-decreasing values, or, with offsets NULL, the msg_len bytes
 * at msgs + i msg_len.  aug is NULL or npoints * aug_len bytes in the memory space of
 * msgs; slice i is hashed in front of message i (the reference's aug argument).  DST
 * is host memory of any length (longer than 255 bytes: replaced once per call by its
 * SHA-256 under "H2C-OVERSIZE-DST-").  dst receives npoints * count elements in the
 * layout above: what the reference's hash_to_field(elems, count G, ..) yields.
 * msm_points_hash: msm_hash_to_field followed by msm_points_map without leaving the
 * device; MSM_H2C_ENCODE selects count = 1 (blst_encode_to_g{1,2}, non-uniform), else
 * count = 2 (blst_hash_to_g{1,2}, the random-oracle variant).
 * u / msgs / aug (one memory space) and dst each in host or device memory (device u and
 * dst 8-byte aligned), on HIP device `device`.
 * npoints == 0: MSM_OK, nothing touched.  MSM_E_ARG, before any device work: a NULL
 * dst, u, or msgs where bytes are needed, group other than 1 or 2, count other than 1
 * or 2, a decreasing offset, unknown flag bits, a host dst overlapping a host source.
 * MSM_E_NODEV: no such device.  MSM_E_HIP: a HIP failure; a host dst is then
 * zero-filled.  Streams as msm_points_to_affine.  On the GPU: csrc/hash_to_curve.hip
 * (DESIGN section 19); chunks of at most 2^18 entries (MSM_H2C_CHUNK=<entries>
 * overrides, read at each call), host memory through two pinned staging buffers per
 * direction.  Thread-safe per call (an engine pool keyed by (device, group), counted by
 * msm_engine_cache_stats(), freed by msm_release_engine_cache()). */
enum { MSM_H2C_ENCODE = 1 }; /* flags of msm_points_hash */
int msm_points_map(int group, int device, void *dst_affine, const void *u, size_t npoints, int count,
                   int src_on_device, int dst_on_device, void *hip_stream);
int msm_hash_to_field(int group, int device, void *dst_elems, const void *msgs, const size_t *offsets, size_t msg_len,
                      const void *aug, size_t aug_len, size_t npoints, const byte *DST, size_t DST_len, int count,
                      int src_on_device, int dst_on_device, void *hip_stream);
int msm_points_hash(int group, int device, void *dst_affine, const void *msgs, const size_t *offsets, size_t msg_len,
                    const void *aug, size_t aug_len, size_t npoints, const byte *DST, size_t DST_len, int flags,
                    int src_on_device, int dst_on_device, void *hip_stream);
/* host only, no device work: DST_prime = DST || I2OSP(len, 1) after the oversize rule.
 * out holds at least 256 bytes; *out_len receives the length.  MSM_E_ARG: NULL out /
 * out_len, NULL DST with DST_len > 0. */
int msm_h2c_dst_prime(byte *out, size_t *out_len, const byte *DST, size_t DST_len);

/* ---- bulk pairings (replaces a loop over the reference's one-pair blst_miller_loop /
 * blst_fp12_mul / blst_final_exp: ref src/pairing.c:181-262 and 371-404) ----
 * A pair is (P, Q): P a G1 and Q a G2 affine point in blst's Montgomery layout (96 and
 * 192 bytes, infinity the all-zero point).  A GT value is a blst_fp12 (576 bytes,
 * canonical).  msm_pairing_segments: dst[j] = blst_final_exp of the product of
 * blst_miller_loop(Q_i, P_i) over offsets[j] <= i < offsets[j + 1], byte for byte;
 * offsets is a HOST array of nsegments + 1 non-decreasing values, or NULL for nsegments
 * segments of one pair each (a plain bulk pairing).  A pair whose P or Q is the all-zero
 * point contributes the factor one at every position; an empty segment gives one.
 * Nothing is validated: the points must be on the curve, and for points outside the
 * prime-order subgroups the value is unspecified (the call completes).  Under
 * MSM_PAIRING_MILLER_ONLY the final exponentiation is skipped: dst[j] is the product of
 * the Miller values, which equals the reference's only up to factors the final
 * exponentiation removes.  dst_fp12 may be NULL when only the verdicts are wanted.
 * is_one (nsegments bytes) and nfail are HOST memory and may be NULL: is_one[j] = 1 when
 * value j is one, *nfail = the number of values that are not; a call that passes either
 * returns only after they are written.  msm_fp12_final_exp: dst[i] = blst_final_exp of
 * the canonical value src[i]; a zero input gives zero (verdict 0), as the reference's
 * blst_final_exp does, and disturbs no other value.
 * p / q (one memory space), src and dst each in host or device memory (device pointers
 * 8-byte aligned), on HIP device `device`.
 * nsegments == 0 / n == 0: MSM_OK, nothing touched.  MSM_E_ARG, before any device work:
 * NULL p / q with pairs to read, NULL src, NULL dst with neither is_one nor nfail, a
 * decreasing offset, unknown flag bits, is_one / nfail under MSM_PAIRING_MILLER_ONLY, a
 * host dst overlapping a host source.  MSM_E_NODEV: no such device.  MSM_E_HIP: a HIP
 * failure; a host dst is then zero-filled, is_one filled with 0 and *nfail set to the
 * number of values.  Streams as msm_points_to_affine.  On the GPU: csrc/pairing.hip
 * (DESIGN section 21); chunks of at most 2^16 pairs (MSM_PAIRING_CHUNK=<pairs>
 * overrides, read at each call; a segment may span chunks), pieces of at most
 * MSM_PAIRING_PIECE=<pairs> pairs, host memory through two pinned staging buffers per
 * lane.  Thread-safe per call (an engine pool keyed by device, counted by
 * msm_engine_cache_stats(), freed by msm_release_engine_cache()). */
enum { MSM_PAIRING_MILLER_ONLY = 1 }; /* flags: skip the final exponentiation */
int msm_pairing_segments(int device, void *dst_fp12, uint8_t *is_one, size_t *nfail, const void *p_affine,
                         const void *q_affine, const size_t *offsets, size_t nsegments, int flags, int src_on_device,
                         int dst_on_device, void *hip_stream);
int msm_fp12_final_exp(int device, void *dst_fp12, uint8_t *is_one, size_t *nfail, const void *src_fp12, size_t n,
                       int src_on_device, int dst_on_device, void *hip_stream);
/* host only: the piece length msm_pairing_segments uses for npairs pairs (MSM_PAIRING_PIECE and
 * MSM_PAIRING_CHUNK as set at the call) */
size_t msm_pairing_piece(size_t npairs);

/* ---- bulk BLS signature verification (replaces a host loop over the reference's
 * blst_core_verify_pk_in_g{1,2} and its blst_pairing_chk_n_aggr_pk_in_g{1,2} /
 * blst_pairing_chk_n_mul_n_aggr_pk_in_g{1,2} / blst_pairing_commit /
 * blst_pairing_finalverify sequences: ref src/aggregate.c:98-339, 390-501, 625-673) ----
 * scheme is the group of the public keys: MSM_SIG_MIN_PK keys in G1, signatures and
 * hashes in G2 (the reference's *_pk_in_g1 calls); MSM_SIG_MIN_SIG keys in G2,
 * signatures and hashes in G1 (*_pk_in_g2).  Every check decides
 *   e(-g, S) prod_i e(PK'_i, H(m_i)) == 1        (min-sig: the sides swapped)
 * with g the generator of the keys' group.  status[j] is a BLST_ERROR value, one byte
 * per check: 0 success, 1 bad encoding, 2 not on curve, 3 not in group, 5 verify fail,
 * 6 public key is infinity.  status and nfail are HOST memory (either may be NULL, not
 * both); *nfail = the number of non-zero statuses; a call returns once they are written.
 * Keys, signatures, msgs, aug and scalars share one memory space (src_on_device);
 * every offsets array and DST are HOST memory.  msgs / msg_offsets / msg_len / aug /
 * aug_len / DST and the flag MSM_H2C_ENCODE are exactly those of msm_points_hash
 * (message i of the call belongs to tuple i).  With MSM_SIG_ENCODED keys and signatures
 * are compressed ZCash entries (48 bytes in G1, 96 in G2); without it blst affine
 * points (96 / 192 bytes, infinity all zero) that are ASSUMED to lie on the curve, as
 * the reference assumes it.
 *
 * msm_sigs_verify: nchecks independent checks; check i has message i, signature i and
 *   the keys pk_offsets[i] .. pk_offsets[i + 1] (pk_offsets NULL: key i alone), which
 *   are summed (FastAggregateVerify); with one key it is blst_core_verify_pk_in_g{1,2}.
 * msm_sigs_aggregate_verify: check j has signature j and the (key, message) tuples
 *   offsets[j] .. offsets[j + 1]: blst_pairing_chk_n_aggr_pk_in_g{1,2} per tuple with
 *   both group checks on and the signature passed with the first tuple, then
 *   blst_pairing_commit and blst_pairing_finalverify(ctx, NULL).  Messages are not
 *   required to be distinct (nor does the reference require it).
 * msm_sigs_batch_verify: check j has the (key, message, signature, scalar) tuples
 *   offsets[j] .. offsets[j + 1]: blst_pairing_chk_n_mul_n_aggr_pk_in_g{1,2} per tuple,
 *   then commit and finalverify.  Scalar i is the low nbits bits of the little-endian
 *   value at scalars + i scalar_stride, with the rules of msm_points_mult; it multiplies
 *   signature i and the G1 side of tuple i (the key in min-pk, the hash in min-sig, as
 *   the reference).  scalars NULL or nbits == 0: the unweighted form.  The caller
 *   supplies the weights, as blst's caller does: they MUST be unpredictable to the
 *   signers (fresh randomness of at least 64 bits per tuple, non-zero), or a batch of
 *   forged signatures can be made to pass.
 * Tuples (keys, messages, signatures, scalars) are indexed from 0; those below
 * offsets[0] are ignored.
 *
 * The status of a check is the code of the FIRST failing step of this sequence.  Per
 * tuple, in order (msm_sigs_verify and msm_sigs_aggregate_verify have one signature,
 * taken with the first tuple):
 *   the signature: with MSM_SIG_ENCODED its uncompress code (1, 2); an infinite
 *     signature is skipped, not rejected; otherwise 3 when it lies outside its group;
 *   then each key of the tuple, in order: its uncompress code; 6 when it is infinite;
 *     3 when it lies outside its group.
 * msm_sigs_verify then gives 6 when the sum of the keys is infinite (an empty set
 * included).  When no step fails: 0 when the pairing product is one, else 5.  A check
 * of the aggregate and batch calls with no tuples gives 5 (the reference's finalverify
 * returns 0 when nothing was aggregated).  One difference, on inputs no honest caller
 * produces: where the signatures of a check sum to infinity, or a weighted point is
 * infinity, the pair is left out of the product (factor one).
 *
 * nchecks == 0: MSM_OK, nothing touched.  MSM_E_ARG, before any device work: NULL
 * status and nfail, a NULL array that is read, a decreasing offset, unknown scheme or
 * flag bits, nbits > 256, a scalar_stride shorter than (nbits + 7) / 8 or above 2^20,
 * misaligned device points (8 bytes; encoded entries 4).  MSM_E_NODEV: no such device.
 * MSM_E_HIP: a HIP failure; every status is then 5 and *nfail the number of checks.
 * Streams as msm_points_to_affine.  On the GPU: csrc/sig_verify.hip (DESIGN section
 * 24): the decode, screen, sum, mult, hash and pairing engines on one stream, the
 * intermediates in device memory; chunks of whole checks of at most 2^16 tuples
 * (MSM_SIGS_CHUNK=<tuples> overrides, read at each call; a longer check is a chunk of
 * its own).  Thread-safe per call (an engine pool keyed by (device, scheme), counted
 * by msm_engine_cache_stats(), freed by msm_release_engine_cache()).
 *
 * msm_points_in_group: in_group[i] = blst_p{1,2}_affine_in_g{1,2}(P_i) for npoints blst
 * affine points in host or device memory; infinity passes; the points are not
 * modified; in_group is HOST memory.  Errors as above (a HIP failure fills in_group
 * with 0); the pool is keyed by (device, group). */
enum { MSM_SIG_MIN_PK = 1, MSM_SIG_MIN_SIG = 2 }; /* scheme */
enum { MSM_SIG_ENCODED = 2 };                     /* flags, beside MSM_H2C_ENCODE */
int msm_sigs_verify(int scheme, int device, uint8_t *status, size_t *nfail, const void *pks, const size_t *pk_offsets,
                    const void *sigs, const void *msgs, const size_t *msg_offsets, size_t msg_len, const void *aug,
                    size_t aug_len, size_t nchecks, const byte *DST, size_t DST_len, int flags, int src_on_device,
                    void *hip_stream);
int msm_sigs_aggregate_verify(int scheme, int device, uint8_t *status, size_t *nfail, const void *pks, const void *sigs,
                              const void *msgs, const size_t *msg_offsets, size_t msg_len, const void *aug,
                              size_t aug_len, const size_t *offsets, size_t nchecks, const byte *DST, size_t DST_len,
                              int flags, int src_on_device, void *hip_stream);
int msm_sigs_batch_verify(int scheme, int device, uint8_t *status, size_t *nfail, const void *pks, const void *sigs,
                          const byte *scalars, size_t nbits, size_t scalar_stride, const void *msgs,
                          const size_t *msg_offsets, size_t msg_len, const void *aug, size_t aug_len,
                          const size_t *offsets, size_t nchecks, const byte *DST, size_t DST_len, int flags,
                          int src_on_device, void *hip_stream);
int msm_points_in_group(int group, int device, uint8_t *in_group, const void *points_affine, size_t npoints,
                        int src_on_device, void *hip_stream);
/* host only, no device work.  msm_sigs_chunk: the tuples per chunk as set at the call.
 * msm_sigs_plan: the chunk of whole checks that starts at check c0 under `chunk` tuples
 * (mode 0 verify, 1 aggregate, 2 batch): *c1 its end, counts = {message rows, keys,
 * signatures, pairing rows}; per pairing row its check (relative to c0) and source (the
 * row's index in the chunk, 0x80000000 the check's signature row); the pairing offsets
 * and, where the mode has them, the segment offsets of the key sums and the signature
 * sums (each checks + 1 values).  Arrays may be NULL; at most `capacity` values are
 * written to each.  msm_sigs_reduce: the statuses of the checks [c0, c1) from the
 * screen's code bytes of their signatures and keys (0, 1, 2, 3, 0x80 infinity), the
 * late bytes (1: the key sum is infinite; may be NULL) and the pairing verdicts. */
size_t msm_sigs_chunk(void);
int msm_sigs_plan(int mode, const size_t *offsets, const size_t *pk_offsets, size_t nchecks, size_t c0, size_t chunk,
                  size_t *c1, size_t counts[4], uint32_t *ent_check, uint32_t *ent_src, size_t *pair_off,
                  size_t *key_off, size_t *sig_off, size_t capacity);
int msm_sigs_reduce(int mode, const size_t *offsets, const size_t *pk_offsets, size_t c0, size_t c1,
                    const uint8_t *sig_codes, const uint8_t *key_codes, const uint8_t *late, const uint8_t *is_one,
                    uint8_t *status);

/* ---- bulk scalar-field arithmetic and batched NTTs (the loops over blst_fr_mul /
 * blst_fr_add / blst_fr_sub a prover runs before it commits: ref src/exports.c
 * blst_fr_*, bindings/blst.h:80-97) ----
 * Elements are 32 bytes: blst_fr (four little-endian 64-bit limbs of a 2^256 mod r,
 * canonical; the default) or blst_scalar (32 little-endian bytes of a).  A blst_fr
 * source must be canonical and nothing is validated.
 *
 * msm_fr_ntt: `batch` transforms over consecutive arrays of n = 2^log_n elements,
 * natural order in and out.  With omega = 7^((r - 1) / 2^32) and omega_n =
 * omega^(2^(32 - log_n)):  forward dst[k] = sum_j src[j] omega_n^(j k);
 * MSM_NTT_INVERSE dst[j] = n^-1 sum_k src[k] omega_n^(-j k).  shift: NULL or one HOST
 * blst_scalar s, 0 < s < r: the forward transform first multiplies src[j] by s^j (it
 * evaluates on the coset s <omega_n>), the inverse multiplies its result j by s^-j.
 * MSM_FR_SRC_SCALAR / MSM_FR_DST_SCALAR select the blst_scalar form on either side,
 * fused into the first load and the last store; a scalar-form source of any 256-bit
 * value is taken mod r, as blst_fr_from_scalar takes it.  log_n = 0 is a copy, or a
 * change of form.  dst == src is allowed (in place).
 * batch == 0: MSM_OK, nothing touched.  MSM_E_ARG, before any device work: NULL dst or
 * src with work to do, log_n above 26 (or batch 2^log_n above 2^40), unknown flag bits,
 * a shift of 0 or >= r, a dst that overlaps src without being equal to it, device
 * pointers not 8-byte aligned.  MSM_E_NODEV: no such device.  MSM_E_HIP: a HIP failure;
 * a host dst is then zero-filled.  Streams and thread safety as msm_points_to_affine
 * (an engine pool keyed by device, counted by msm_engine_cache_stats(), freed by
 * msm_release_engine_cache()).
 * On the GPU: csrc/fr_ntt.hip.  Stockham passes planned by
 * csrc/ntt_plan.hpp, each workgroup running its radix in LDS on a tile of 2^10 elements
 * (MSM_NTT_TILE=<log2> in 2..11 overrides, read at each call); no pass only permutes.
 * Chunks of whole transforms of at most 2^20 elements (MSM_NTT_CHUNK=<elements>
 * overrides, read at each call; a longer transform is a chunk of its own); host memory
 * goes through the pinned staging of the other bulk calls.
 *
 * msm_fr_op: dst[i] = a[i] op b[i], byte for byte what blst_fr_add / _sub / _mul / _sqr /
 * blst_fr_cneg(.., 1) / blst_fr_inverse / blst_fr_from_scalar / blst_scalar_from_fr give.
 * b is ignored by the one-operand ops; with MSM_FR_B_ONE it holds ONE element, used for
 * every a[i].  a and b are on the side src_on_device names.  dst may equal a or b.
 * MSM_FR_INV is one batch inversion per chunk, the product tree of msm_points_to_affine
 * over Fr; the inverse of zero is zero (as blst_fr_inverse gives) and a zero disturbs
 * no other element.  n == 0: MSM_OK.  MSM_E_ARG: an unknown op or flag bit, a NULL
 * array that is read or written, a dst that overlaps a or b without being equal to it,
 * misaligned device pointers.  Other errors, streams and the pool as msm_fr_ntt. */
typedef struct { limb_t l[256 / 8 / sizeof(limb_t)]; } blst_fr; /* blst.h:57 */
enum { MSM_NTT_INVERSE = 1, MSM_FR_SRC_SCALAR = 2, MSM_FR_DST_SCALAR = 4 };
int msm_fr_ntt(int device, void *dst, const void *src, size_t log_n, size_t batch, const byte *shift, int flags,
               int src_on_device, int dst_on_device, void *hip_stream);
enum { MSM_FR_ADD, MSM_FR_SUB, MSM_FR_MUL, MSM_FR_SQR, MSM_FR_NEG, MSM_FR_INV, MSM_FR_FROM_SCALAR, MSM_FR_TO_SCALAR };
enum { MSM_FR_B_ONE = 1 }; /* b holds ONE element, used for every a[i] */
int msm_fr_op(int device, int op, void *dst, const void *a, const void *b, size_t n, int flags, int src_on_device,
              int dst_on_device, void *hip_stream);
/* host only, no device work.  msm_fr_root_of_unity: omega_n for n = 2^log_n, log_n <= 32,
 * as a blst_fr.  msm_ntt_plan: the passes of a transform under the MSM_NTT_TILE set at
 * the call: *npasses their number (0 for log_n = 0) and log_radix[i] the log2 of the
 * radix of pass i (at most `capacity` written; may be NULL); log_n above 26: MSM_E_ARG. */
int msm_fr_root_of_unity(size_t log_n, blst_fr *out);
int msm_ntt_plan(size_t log_n, int *npasses, int log_radix[], int capacity);
/* diagnostic: register-resident Fr products per second on `device` (out[0]) and the
 * milliseconds the measurement took (out[1]) */
int msm_fr_probe(int device, double out[2]);

/* ---- evaluation-form polynomials and KZG (what a blob proof or a PLONK opening is made
 * of: evaluate outside the domain, divide by (X - z), commit the quotient, check it) ----
 * msm_fr_eval_quotient.  polys: `count` consecutive arrays of n = 2^log_n blst_fr, the
 * values of polynomial j (degree < n) on the domain of msm_fr_ntt, omega_n =
 * msm_fr_root_of_unity(log_n): position i holds the value at x_i = omega_n^i, or with
 * MSM_POLY_BITREV at omega_n^bitrev(i, log_n) (the order of EIP-4844 blobs).  z: count
 * blst_fr, one point per polynomial (polys and z on the side src_on_device names).
 * y[j] (count blst_fr, canonical) is the value of polynomial j at z[j].  q may be NULL;
 * otherwise it receives count n elements, the values of (f_j - y_j) / (X - z_j) on the
 * same domain in the same order, as blst_fr or, under MSM_FR_DST_SCALAR, as blst_scalar
 * bytes (the form rides on the store; it is what an MSM reads).  y and q are on the
 * side dst_on_device names; q == polys is allowed (in place).  Elements must be
 * canonical and nothing is validated.
 * With d_i = (z - x_i)^-1, the inverse of zero taken as zero (the MSM_FR_INV
 * convention), S = sum f_i x_i d_i and T = sum x_i d_i:
 *   z outside the domain:  y = (z^n - 1) n^-1 S,  q_i = (y - f_i) d_i
 *   z = x_m:               y = f_m,  q_i = (y - f_i) d_i for i != m,  q_m = z^-1 (S - y T).
 * count == 0: MSM_OK, nothing touched.  MSM_E_ARG, before any device work: NULL y, polys
 * or z with work to do, log_n above 26 (or count 2^log_n above 2^40), unknown flag bits,
 * a q that overlaps polys without being equal to it (or y / z overlapping another
 * array), device pointers not 8-byte aligned.  MSM_E_NODEV: no such device.  MSM_E_HIP:
 * a HIP failure; host y and q are then zero-filled.  Streams and thread safety as
 * msm_points_to_affine (an engine pool keyed by device, counted by
 * msm_engine_cache_stats(), freed by msm_release_engine_cache()).
 * On the GPU: csrc/fr_poly.hip.  A workgroup inverts a tile of 2^10
 * elements together (MSM_POLY_TILE=<log2> in 2..10 overrides, read at each call):
 * prefix products per lane, a product tree over the lanes in LDS, one Fermat chain; the
 * tiles of all polynomials of a chunk run side by side; a second kernel adds the
 * partial sums of a polynomial's tiles and forms y, a third writes q.  Chunks of whole
 * polynomials of at most 2^20 elements (MSM_POLY_CHUNK=<elements> overrides, read at
 * each call; a longer polynomial is a chunk of its own); host memory goes through the
 * pinned staging of the other bulk calls.
 *
 * msm_kzg_*: a context over one structured reference string in LAGRANGE form: n =
 * 2^log_n G1 affine points L_i = [l_i(tau)]G1, l_i the Lagrange basis of the domain
 * above, in natural order or, with MSM_POLY_BITREV in `flags` (fixed at creation), in
 * bit-reversed order -- the order of the polynomials it is used with.  log_n <= 20.
 * srs_lagrange_g1: host or device memory (srs_on_device), copied; tau_g2: one HOST
 * blst_p2_affine, [tau]G2.  The context owns an msm_ctx (plain Pippenger) over the SRS.
 *   commit: dst[j] = sum_i f_j[i] L_i = [f_j(tau)]G1, affine (all zero: infinity), for
 *     `count` polynomials of n blst_fr.  The polynomials are turned into blst_scalar
 *     bytes on the device (MSM_FR_TO_SCALAR) and summed by one msm_ctx_mult_batch per
 *     chunk of MSM_POLY_CHUNK elements.
 *   open: y[j] = f_j(z[j]) and proofs[j] = [q_j(tau)]G1 for q_j = (f_j - y_j) / (X - z_j):
 *     msm_fr_eval_quotient under MSM_FR_DST_SCALAR into a device buffer, then the same
 *     batch MSM; nothing of the quotient crosses to the host.  polys and z on the side
 *     src_on_device names, proofs and y on the side dst_on_device names.
 *   verify: `count` tuples (C_j, z_j, y_j, pi_j): commitments and proofs blst_p1_affine,
 *     z and y blst_fr, all on the side src_on_device names.  weights == NULL: ok[j] = 1
 *     iff e(C_j - [y_j]G1 + [z_j]pi_j, -G2) e(pi_j, [tau]G2) = 1 (G1, G2 the blst
 *     generators): `count` verdicts; batch_offsets is ignored.  With weights (the
 *     contract of msm_sigs_batch_verify: r_j the low nbits bits of the little-endian
 *     string at weights + j weight_stride, nbits <= 256, taken mod r; weights is
 *     always a HOST array), batch b covers
 *     the tuples batch_offsets[b] .. batch_offsets[b + 1] (a HOST array of nbatches + 1
 *     non-decreasing values, the last at most count; NULL: one batch of all tuples) and
 *     ok[b] = 1 iff e(sum r_j (C_j - [y_j]G1 + [z_j]pi_j), -G2) e(sum r_j pi_j, [tau]G2)
 *     = 1: one check of two pairs per batch; an empty batch gives 1.  The three scalars
 *     of a tuple (r_j, -r_j y_j, r_j z_j) are computed on the HOST; the point sums run
 *     through msm_points_msm_segments and the checks through msm_pairing_segments.  An
 *     all-zero proof is infinity, a legal input (a constant polynomial opens to it).
 *     Points are not validated: they must be on the curve and in the prime-order
 *     subgroups (chain msm_points_decode / msm_points_in_group first).  ok (host, one
 *     byte per verdict) and nfail (the number of zeros) may each be NULL, not both; the
 *     call returns with them written.
 * Every call is ordered on hip_stream; a call with a host destination returns with the
 * data in place, one with a device destination after the batch MSM has finished (its
 * Jacobians pass through the host, as msm_ctx_mult_batch returns them).  A context
 * serves one call at a time.  count == 0: MSM_OK, nothing touched.  MSM_E_ARG, before
 * any device work: a NULL context or array that is read or written, log_n above 20,
 * unknown flag bits, misaligned device pointers, nbits > 256, a weight_stride shorter
 * than (nbits + 7) / 8, a decreasing batch offset or one past count.  MSM_E_NODEV: no
 * such device.  MSM_E_HIP: a HIP failure; host outputs are then zero-filled, ok filled
 * with 0 and *nfail set to the number of verdicts.
 * msm_kzg_ctx_create_monomial: the same context from an SRS in MONOMIAL form, as a
 * trusted setup publishes it: srs_monomial_g1 holds the n points [tau^i]G1, i in natural
 * order, host or device memory.  The context is the one msm_kzg_ctx_create builds from
 * the inverse msm_points_ntt (below) of those points, bit-reversed when `flags` has
 * MSM_POLY_BITREV; the transform runs on the device and its result never visits the
 * host.  Guards and codes as msm_kzg_ctx_create; returns after the transform is done.
 * Out of scope: EIP-4844's Fiat-Shamir challenge and big-endian field bytes,
 * multi-point openings (FK20), G2 commitments. */
enum { MSM_POLY_BITREV = 8 }; /* shares the flag word with MSM_FR_DST_SCALAR (4) */
int msm_fr_eval_quotient(int device, void *y, void *q, const void *polys, const void *z, size_t log_n, size_t count,
                         int flags, int src_on_device, int dst_on_device, void *hip_stream);
typedef struct msm_kzg_ctx msm_kzg_ctx;
int msm_kzg_ctx_create(msm_kzg_ctx **ctx, int device, size_t log_n, const void *srs_lagrange_g1, int srs_on_device,
                       const void *tau_g2, int flags, void *hip_stream);
void msm_kzg_ctx_destroy(msm_kzg_ctx *ctx);
int msm_kzg_commit(msm_kzg_ctx *ctx, void *dst_affine, const void *polys, size_t count, int src_on_device,
                   int dst_on_device, void *hip_stream);
int msm_kzg_open(msm_kzg_ctx *ctx, void *proofs_affine, void *y, const void *polys, const void *z, size_t count,
                 int src_on_device, int dst_on_device, void *hip_stream);
int msm_kzg_verify(msm_kzg_ctx *ctx, uint8_t *ok, size_t *nfail, const void *commitments, const void *z,
                   const void *y, const void *proofs, size_t count, const byte *weights, size_t nbits,
                   size_t weight_stride, const size_t *batch_offsets, size_t nbatches, int src_on_device,
                   void *hip_stream);
int msm_kzg_ctx_create_monomial(msm_kzg_ctx **ctx, int device, size_t log_n, const void *srs_monomial_g1,
                                int srs_on_device, const void *tau_g2, int flags, void *hip_stream);

/* ---- NTTs over group elements (the change of basis of an SRS or of committed data: the
 * loop over blst_p{1,2}_mult and blst_p{1,2}_add_or_double a setup or an FK20 prover
 * writes; no single reference counterpart) ----
 * msm_points_ntt: `batch` transforms over consecutive arrays of n = 2^log_n affine points
 * (blst_p1_affine / blst_p2_affine, group 1 / 2; the all-zero point is infinity, legal on
 * input and on output), on the domain of msm_fr_ntt, omega_n = msm_fr_root_of_unity(log_n):
 *   forward            dst[k] = sum_j [omega_n^(j k)] src[j]
 *   MSM_NTT_INVERSE    dst[j] = [n^-1] sum_k [omega_n^(-j k)] src[k]
 *   MSM_POLY_BITREV    the evaluation side is in bit-reversed order: the inverse writes
 *                      result j at position bitrev(j, log_n), the forward transform reads
 *                      its source element j at position bitrev(j, log_n); forward after
 *                      inverse, both under the flag, is the identity, and the inverse of a
 *                      monomial SRS is what msm_kzg_ctx_create(.., MSM_POLY_BITREV) wants
 * log_n = 0 is a copy (through the canonical form).  dst may equal src.  log_n <= 24.
 * The points MUST lie in the prime-order subgroup; they are not validated (chain
 * msm_points_decode / msm_points_in_group first).  Outside the subgroup the result is
 * unspecified: the factorisation of the twiddles into levels holds mod r only.  Within
 * it every output is the canonical affine point, byte for byte.
 * On the GPU: csrc/points_ntt.hip on the plan of csrc/points_ntt_plan.hpp (DESIGN section
 * 31): radix-2 decimation in frequency on xyzz points; per level one general add and one
 * subtraction per butterfly, then the 255-bit signed-window ladder of msm_points_mult
 * on the difference with the twiddle as its scalar (the last level has none); the inverse
 * adds one ladder per element for n^-1; one batch inversion at the end.  Chunks of whole
 * transforms of at most 2^20 points (MSM_POINTS_NTT_CHUNK=<points> overrides; a longer
 * transform is a chunk of its own); the butterflies of a chunk's level run in slices of
 * at most 2^18 (MSM_POINTS_NTT_SLICE=<butterflies> overrides; both read at each call).
 * Twiddle tables (16 n + 32 bytes) are kept per engine and log_n; engines are pooled per
 * (device, group) and counted by msm_engine_cache_stats().  Host memory goes through the
 * pinned staging of the other bulk calls; streams as msm_points_to_affine.
 * batch == 0: MSM_OK, nothing touched.  MSM_E_ARG, before any device work: a NULL
 * pointer with work to do, a group other than 1 or 2, log_n > 24 or batch n > 2^40,
 * unknown flag bits, a dst that overlaps src without equalling it, misaligned device
 * pointers.  MSM_E_NODEV: no such device.  MSM_E_HIP: a HIP failure; a host dst is then
 * zero-filled.
 * msm_points_ntt_model (host only, no device work): the same plan -- maps, levels with
 * their pairs and exponents, the n^-1 pass, slices and chunks under the two overrides --
 * run on blst_fr elements in place of points (the group Z_r), so the schedule can be
 * checked on the CPU against any Fr NTT.  log_n <= 16, else MSM_E_ARG; dst may be src. */
int msm_points_ntt(int group, int device, void *dst_affine, const void *src_affine, size_t log_n, size_t batch,
                   int flags, int src_on_device, int dst_on_device, void *hip_stream);
int msm_points_ntt_model(size_t log_n, int flags, blst_fr *dst, const blst_fr *src);

/* host setup logic of the CHES method (no device work):
 * bucket set of ref auxiliaryfunc.h:257-288 (returns |B|; out may be NULL) */
size_t msm_ches_bucket_set(int q, int a_h, int *out, size_t cap);
/* digit hash of ref main_p1.cpp:140-152, q+1 entries in the blst.h:253 layout */
int msm_ches_digit_table(int q, int a_h, digit_decomposition *out);

/* ---- boundary helpers (host; no blst symbols are redefined) ---- */
void msm_gen_scalars(byte *out32, size_t n, uint64_t seed);         /* BASELINE.md sec.3 SplitMix64 */
void msm_p1_fixed_points(blst_p1_affine *out, size_t n);            /* P_i = 2^(i+1) G1 (main_p1.cpp:52-66) */
void msm_p2_fixed_points(blst_p2_affine *out, size_t n);
/* P_{start+i} = 2^(start+i+1) G for i < n: the shard of the same point sequence */
void msm_p1_fixed_points_range(blst_p1_affine *out, size_t start, size_t n);
void msm_p2_fixed_points_range(blst_p2_affine *out, size_t start, size_t n);
void msm_p1_to_affine(blst_p1_affine *out, const blst_p1 *in);      /* e1.c:80-92 */
void msm_p2_to_affine(blst_p2_affine *out, const blst_p2 *in);
void msm_p1_compress(byte out[48], const blst_p1 *in);              /* e1.c:225-234 */
void msm_p2_compress(byte out[96], const blst_p2 *in);
void msm_p1_add(blst_p1 *out, const blst_p1 *a, const blst_p1 *b);  /* Jacobian, doubling aware */
void msm_p2_add(blst_p2 *out, const blst_p2 *a, const blst_p2 *b);

/* ---- device self-test entry points (parity tests of the Fp/Fp2/xyzz layers) ----
 * op: 0 mul, 1 add, 2 sub, 3 sqr; values in blst Montgomery layout */
int msm_test_field(int group, int op, const limb_t *a, const limb_t *b, limb_t *out, size_t n);
/* nseq sequences of len ops (point index | sign<<31, 0xffffffff = skip) -> per sequence
 * two blst Jacobians: acc and acc+acc (via the xyzz+xyzz path) */
int msm_test_xyzz(int group, const void *points_affine, size_t npoints, const uint32_t *ops, int len, size_t nseq,
                  void *out);
/* one operation of the Fp12 tower (csrc/fp12l.hpp) on n values, one lane pair each, on
 * device 0, synchronously.  op: 0 out = a b, 1 a^2, 2 a (x + y v + z v w) with x, y, z the
 * coefficients 0, 1, 4 of b, 3 conj(a), 4 a^(p^k) (k = 1 .. 3), 5 1 / a, 6 a^(2^k) by k
 * cyclotomic squarings held in registers (a unitary, k = 1 .. 64), 7 / 8 the doubling /
 * addition step of the Miller loop with its line: a = (X, Y, Z, qx, qy, unused), out =
 * (X3, Y3, Z3, l0, l1, l2).  alias: 0 a destination of its own, 1 the destination is a
 * (ops 0 .. 4 and 6), 2 it is b (op 0).  raw 0: a, b, out are blst Fp12 values (576
 * bytes; in through the arithmetic of msm_fp12_final_exp, out canonical); raw 1: the
 * stored form, 672 bytes: six Fp2, each c0 | c1, 14 little-endian 28-bit limbs in
 * uint32 of value 2^392 mod p, in and out untouched, so the caller chooses the
 * representative (class S: limbs 0 .. 12 below 2^28, value below 2p) and sees the
 * result's.  b is read by ops 0 and 2 only.  n == 0: MSM_OK.  MSM_E_ARG, before any
 * device work: an unknown op, alias or raw, k out of range, a NULL array that is used. */
int msm_test_fp12(int op, int k, int alias, int raw, const void *a, const void *b, void *out, size_t n);
/* one operation of the field and curve layers under every product kernel (csrc/fp.hpp,
 * fp2l.hpp, ec.hpp, coop.hpp) on n values, on device 0, synchronously, on raw stored
 * words: an element is 14 little-endian 28-bit limbs in uint32 (Fp) or two of them, c0 |
 * c1 (Fp2, Fp2L), of value 2^392 mod p, in and out untouched, so the caller chooses the
 * representative (any limbs the op's range class allows, lazy ones included) and sees
 * the result's.
 * field: 0 Fp, one lane per value; 1 Fp2, one lane per value; 2 Fp2L, value i on lanes 2i
 *   (c0) and 2i + 1 (c1) of 64-thread blocks, 32 values per block.
 * form: 0 split Montgomery columns, 1 the single chain (MulChain; Fp only, ops marked *).
 * op, with the elements it reads per value (in = n x that many, value after value):
 *    0 f_mul* (a, b)          1 f_mul_bs* (a, b)        2 f_sqr* (a)
 *    3 f_mul_sub* (a, b, c, d) = a b - c d              4 f_mul_sub_bs* (a, b, c, d)
 *    5 f_add (a, b)           6 f_sub4 (a, b)           7 f_sub16 (a, b)
 *    8 fp_sub<8> (a, b)       9 fp_sub<32> (a, b), both per component
 *   10 f_sub_2x (a, b, c) = a + 8p - b - 2c            11 f_neg4 (a)    12 f_mul3 (a)
 *   13 f_norm (a)            14 f_nred (a)             15 f_one ()
 *   16 f_is_zero_exact (a)   17 f_is_zero_S (a): out is one uint32 per value, 0 or 1
 *      (Fp2L: the even lane's verdict, which is the pair's)
 *   Fp only: 18 fp_mul2* (a, b, c, d) = a b + c d      19 fp_mul4* (a .. h) = a b + c d +
 *      e f + g h             20 fp_red (a)             21 fp_cneg4 (a; flag bit 0)
 *      22 fp_canon (a)       23 fp_csub_p (a)
 *   curve ops, points as stored (x, y, zzz, zz), out = the xyzz result:
 *   24 xyzz_madd* (acc, then the affine x2, y2; flags bit 0: neg, bit 1: acc_affine -- the
 *      accumulator is then xyzz_from_aff of (acc.x, acc.y) with sign bit 2, zzz and zz
 *      unread; the flags of a value hold for both lanes of an Fp2L pair)
 *   25 xyzz_add* (acc, b), the field's default instantiation   26 xyzz_add_u1s1* (acc, b)
 *   27 xyzz_dbl* (a)
 *   28 the cooperative add of coop.hpp through the reductions' own kernels: field 0
 *      k_pair_step_c<1>, field 2 k_pair_step_c2p, out[i] = in[2i] + in[2i + 1] (field 1
 *      has no such kernel: MSM_E_ARG)
 *   Every combination above is built, none was left out for its registers, except op 4
 *   on field 1: fp.hpp has no f_mul_sub_bs over the one-lane Fp2 (MSM_E_ARG).
 * flags: one uint32 per value, read by ops 21 and 24 only.  out: cap >= n slots (an
 * element, a point or a word each); all cap slots go to the device as the caller filled
 * them and come back, so a slot from n on returns as it went in unless a kernel wrote
 * past its n.  n == 0: MSM_OK.  MSM_E_ARG, before any device work: an unknown field, form
 * or op, form 1 for an op or field without it, an Fp-only op on another field, cap < n,
 * a NULL array that is used (in unless the op reads nothing, flags for ops 21 and 24,
 * out). */
int msm_test_fp_ops(int field, int form, int op, const uint32_t *in, const uint32_t *flags, uint32_t *out, size_t n,
                    size_t cap);

#ifdef __cplusplus
}
#endif
#endif
