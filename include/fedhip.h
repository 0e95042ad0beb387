/*
 * fedhip.h — C ABI of libfedhip.so, the MI355X (gfx950) hot path for
 * per-client CNN training, update-level differential privacy and FedAvg.
 *
 * Every entry point:
 *   - returns FH_OK (0) or a negative FH_E_* code; fh_last_error() gives a
 *     thread-local message for the last failure on the calling thread;
 *   - takes caller-owned DEVICE pointers (fp32 unless stated), contiguous,
 *     with element strides spelled out; no hidden allocation, no host sync;
 *   - launches on `stream` (a hipStream_t passed as void*; NULL = default).
 *
 * "Packed" tensors hold many simulated clients: client slot z of a tensor
 * `t` with client stride `t_cs` starts at t + z * t_cs.  Clients are packed
 * into slots sorted by descending step count, so the clients still active at
 * a given step are always the prefix [0, nclients).  `counts[z]` (device
 * int32, may be NULL = all `batch` valid) is the number of valid images of
 * client z in this step — the reference's partial last batch
 * (DataLoader drop_last=False, src/shared/training.py:184).
 *
 * Reference interfaces replaced (file:line in the reference repository):
 *   fh_fedavg_weighted_sum   src/aggregation/fedavg.py:267-289 (_weighted_average)
 *   fh_update_stats          src/shared/validation.py:72-91   (_validate_model_weights)
 *   fh_dp_delta_sqnorm       src/shared/privacy.py:119-123    (GradientClipper norm)
 *                            + src/client/federated_trainer.py:438-443 (delta)
 *   fh_dp_clip_coef          src/shared/privacy.py:123-140, 209 (clip decision, sigma)
 *   fh_dp_apply              src/shared/privacy.py:127-133, 212, 244-245
 *                            + src/client/federated_trainer.py:454-459
 *   fh_sgd_step / fh_adam_step   src/shared/training.py:244-255 + torch.optim
 *   fh_conv2d_* / fh_linear_*    nn.Conv2d / nn.Linear in src/shared/models_pytorch.py
 *   fh_bn_*                  nn.BatchNorm2d (models_pytorch.py:108-120, 176-187)
 *   fh_maxpool2_*            nn.MaxPool2d(2,2) (models_pytorch.py:72,123)
 *   fh_dropout_*             nn.Dropout (models_pytorch.py:75,124)
 *   fh_ce_fwd_bwd            nn.CrossEntropyLoss + metrics (training.py:90,193,200-203)
 *   fh_eval_metrics          LocalTrainer.evaluate_model metrics (training.py:307-360)
 *   fh_quantize_rows         QuantizationCompressor (compression.py:123-247)
 *   fh_topk_rows             TopKSparsificationCompressor (compression.py:250-368)
 *   fh_ef_fold / fh_ef_topk_finish / fh_ef_quant_finish / fh_squant_rows
 *                            not in the reference (error feedback, stochastic rounding)
 *   fh_topk_pack_rows / fh_sparse_validate / fh_sparse_unpack_rows / fh_sparse_fedavg
 *                            TopKSparsificationCompressor's {'values', 'indices'} payload
 *                            (compression.py:262-297, 346-365) and FedAvg straight from it
 *   fh_quant_pack_rows / fh_quant_validate / fh_quant_unpack_rows / fh_quant_fedavg
 *                            QuantizationCompressor's uint8 codes + quantization_params payload
 *                            (compression.py:138-172, 230-244), bit-packed, and FedAvg straight
 *                            from it
 */
#ifndef FEDHIP_H_
#define FEDHIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FH_OK 0
#define FH_E_INVALID (-1)     /* bad argument / shape */
#define FH_E_LAUNCH (-2)      /* HIP launch or runtime failure */
#define FH_E_UNSUPPORTED (-3) /* shape/config outside what the kernels cover */

const char* fh_last_error(void);
int fh_version(void);

/* ---------------- FedAvg (fedavg.py:267-289) ------------------------------
 * out[j] = (accumulate ? out[j] : 0) + sum_{k=0..C-1} fl32(w[k]) * rows[idx[k]*row_stride + j]
 * evaluated sequentially in k with a rounded multiply followed by a rounded
 * add (never a fused multiply-add): bit-exact with the reference's
 * `aggregated[l] += weight * layer` loop over the client list.
 * row_index (device int32[C]) may be NULL (identity); weights: device float[C]. */
int fh_fedavg_weighted_sum(const float* rows, int64_t row_stride, const int32_t* row_index,
                           const float* weights, int32_t num_clients, int64_t P, float* out,
                           int32_t accumulate, void* stream);

/* Per client, per parameter tensor (segment [seg_off[t], seg_off[t+1]) of a row):
 * max |w| and a non-finite flag (validation.py:81-91). seg_offsets: device int64[nseg+1]. */
int fh_update_stats(const float* rows, int64_t row_stride, int32_t num_clients,
                    const int64_t* seg_offsets, int32_t nseg, float* seg_absmax,
                    int32_t* seg_nonfinite, void* stream);

/* ---------------- Byzantine-robust aggregation (no reference counterpart) --
 * Coordinate-wise trimmed mean (Yin et al. 2018).  For each coordinate j independently take
 * the C values rows[idx[k]*row_stride + j] (row_index may be NULL: identity) and order them
 * by the total order on the 32-bit key
 *     key(x) = bits(x) ^ (sign(x) ? 0xFFFFFFFF : 0x80000000),  compared as unsigned,
 * after every NaN (either sign, any payload) has been mapped to one key above +Inf:
 *     -Inf < ... < -0 < +0 < ... < +Inf < NaN.
 * With the sorted values s[0..C-1],
 *     out[j] = (((s[t] + s[t+1]) + ...) + s[C-1-t]) / (float)(C - 2t),   t = trim,
 * fp32 additions in ascending sorted order, one IEEE fp32 division, no FMA; a NaN result is
 * written as the one quiet NaN 0x7FC00000.  The result does not depend on the row order,
 * bit for bit.  Up to `trim` NaN or +-Inf rows per coordinate are discarded; more propagate.
 * The median is trim = (C-1)/2: s[mid] / 1.0f for odd C, (s[C/2-1] + s[C/2]) / 2.0f for even.
 * Requires 1 <= C <= 64 and 0 <= 2*trim < C (FH_E_INVALID otherwise); P == 0 is a no-op.
 * No workspace.  16-byte loads when row_stride % 4 == 0 and rows / out are 16-byte aligned;
 * a scalar path with the same bits covers everything else and the P % 4 tail. */
int fh_trimmed_mean_rows(const float* rows, int64_t row_stride, const int32_t* row_index,
                         int32_t num_clients, int32_t trim, int64_t P, float* out, void* stream);

/* Pairwise squared distances of client rows (the input of Krum / multi-Krum, Blanchard et
 * al. 2017):  dist[a][b] = sum_j ((double)(x_a[j] - x_b[j]))^2  with x_k = rows[idx[k]*
 * row_stride + .]: one rounded fp32 subtraction, square and sum in fp64, computed from the
 * differences directly (never ||a||^2 + ||b||^2 - 2ab, which cancels for rows that sit
 * within one update of each other).  dist: device double[C][C], symmetric, zero diagonal.
 * No atomics: each workgroup writes the partials of its chunk of coordinates for all
 * C(C-1)/2 pairs to `workspace` (>= fh_pairwise_sqdist_workspace(C, P) bytes) and a second
 * launch adds them in chunk order, so the bits are the same on every run.  2 <= C <= 64. */
size_t fh_pairwise_sqdist_workspace(int32_t num_clients, int64_t P);
int fh_pairwise_sqdist(const float* rows, int64_t row_stride, const int32_t* row_index,
                       int32_t num_clients, int64_t P, void* workspace, size_t ws_bytes,
                       double* dist, void* stream);

/* ---------------- secure aggregation (no reference counterpart) ------------
 * Pairwise-masked fixed-point rows in the ring Z/2^32 (Bonawitz et al., CCS 2017).  Both entry
 * points work on mask terms (key: uint64, sign: int32; > 0 adds, < 0 subtracts, 0 skips the
 * term).  With the launch-wide `nonce`, a term's mask word for coordinate j is
 *     m(key, j) = word (j % 4) of Philox4x32-10(seed = key, ctr_hi = nonce, ctr_lo = j / 4),
 * words in the order .x .y .z .w.  Who shares which key is the caller's protocol.
 *
 * fh_secagg_encode_mask_rows: for each row z < num_rows and coordinate j < P, with
 * x = rows[idx[z]*row_stride + j] (row_index may be NULL: identity),
 *     v = weights ? fl32(weights[z] * x) : x          one rounded fp32 multiply, never fused
 *     r = rint((double)v * 2^frac_bits)               exact product, round to nearest even
 *     NaN -> r = 0;  r > qmax -> qmax;  r < -qmax -> -qmax;  each adds 1 to clipped[z]
 *     out[z*out_stride + j] = (uint32)(int32)r + sum_t sign[z][t] * m(key[z][t], j)  mod 2^32
 * term_keys / term_signs: device [num_rows][nterms]; weights: device float[num_rows] or NULL;
 * clipped: device int32[num_rows] or NULL, ADDED to (the caller zeroes it) with one integer
 * atomic per workgroup, so the count is the same on every run.  Requires 0 <= frac_bits <= 30,
 * 1 <= qmax <= 2^31 - 1, 0 <= nterms <= 64, 1 <= num_rows (FH_E_INVALID otherwise); P == 0 is
 * a no-op.  No workspace.  16-byte loads and stores when both strides % 4 == 0 and rows / out
 * are 16-byte aligned; a scalar path with the same bits covers everything else and the P % 4
 * tail. */
int fh_secagg_encode_mask_rows(const float* rows, int64_t row_stride, const int32_t* row_index,
                               const float* weights, int32_t num_rows, int64_t P,
                               int32_t frac_bits, int32_t qmax, const uint64_t* term_keys,
                               const int32_t* term_signs, int32_t nterms, uint64_t nonce,
                               uint32_t* out, int64_t out_stride, int32_t* clipped, void* stream);

/* The server's side: sum the masked rows, remove the terms that did not cancel (pair masks
 * between surviving and dropped clients, the survivors' self masks) and decode:
 *     acc[j]     = sum_k masked[idx[k]*stride + j] - sum_t sign[t] * m(key[t], j)   mod 2^32
 *     sum_out[j] = acc[j]
 *     out[j]     = (float)((double)(int32)acc[j] * 2^-frac_bits)      one rounding, to fp32
 * term_keys / term_signs: device [nterms], nterms >= 0; out (fp32) and sum_out (uint32) may
 * each be NULL but not both; 1 <= num_rows; 0 <= frac_bits <= 30; P == 0 is a no-op.  Sums in
 * the ring do not depend on the order of rows or terms.  Paths as above. */
int fh_secagg_sum_decode(const uint32_t* masked, int64_t stride, const int32_t* row_index,
                         int32_t num_rows, int64_t P, const uint64_t* term_keys,
                         const int32_t* term_signs, int32_t nterms, uint64_t nonce,
                         int32_t frac_bits, float* out, uint32_t* sum_out, void* stream);

/* ---------------- adaptive server optimizers (no reference counterpart) ----
 * Reddi et al., "Adaptive Federated Optimization" (ICLR 2021): the server steps the global
 * model along the pseudo-gradient d = aggregate - global with moments m, v kept across rounds.
 * Per coordinate j; every operation is one rounded fp32 operation, never fused; sqrtf and / are
 * IEEE correctly rounded; denormals are kept:
 *     a    = weights ? (((0 + w[0]*x_0[j]) + w[1]*x_1[j]) + ...)   exactly fh_fedavg_weighted_sum
 *                    : x_0[j]          weights NULL: num_clients must be 1, the row IS the aggregate
 *            x_k = rows[idx[k]*row_stride + j], row_index NULL = identity
 *     d    = a - g                                             g = global[j]
 *     omb1 = 1.0f - beta1,  omb2 = 1.0f - beta2                computed once, in fp32
 *     MOMENTUM: m' = (beta1*m) + d          g' = g + server_lr*m'     v not read or written (may be NULL)
 *     others:   m' = (beta1*m) + (omb1*d)
 *               d2 = d*d
 *       ADAGRAD v' = v + d2
 *       ADAM    v' = (beta2*v) + (omb2*d2)
 *       YOGI    t  = v - d2;  s = t>0 ? 1.0f : t<0 ? -1.0f : 0.0f (NaN t: 0);  v' = v - ((omb2*d2)*s)
 *               g' = g + server_lr * ( m' / (sqrtf(v') + tau) )
 * g', m' and v' are stored in place; any NaN is stored as the one quiet NaN 0x7FC00000.  No bias
 * correction (the paper uses none).  The initial state is the caller's: m = 0, v = tau^2.
 * FH_E_INVALID for: rule outside 0..3; num_clients < 1; weights == NULL with num_clients != 1;
 * P < 0; null rows / global / m; null v for rules 1..3; tau < 0 or a non-finite server_lr /
 * beta / tau.  P == 0 is a no-op.  No workspace.  16-byte loads and stores when row_stride % 4
 * == 0 and rows, global, m and v are 16-byte aligned; a scalar path with the same bits covers
 * everything else and the P % 4 tail.  Reads (C+3)*P floats and writes 3*P ((C+2)*P and 2*P
 * for MOMENTUM). */
#define FH_SOPT_MOMENTUM 0   /* FedAvgM  */
#define FH_SOPT_ADAGRAD  1   /* FedAdagrad */
#define FH_SOPT_ADAM     2   /* FedAdam  */
#define FH_SOPT_YOGI     3   /* FedYogi  */
int fh_server_opt_step(const float* rows, int64_t row_stride, const int32_t* row_index,
                       const float* weights, int32_t num_clients, int64_t P,
                       float* global, float* m, float* v, int32_t rule,
                       float server_lr, float beta1, float beta2, float tau, void* stream);

/* ---------------- FedNova normalised averaging (no reference counterpart) --
 * Wang et al., "Tackling the Objective Inconsistency Problem in Heterogeneous Federated
 * Optimization" (NeurIPS 2020): with FedAvg weights p_k and local step counts a_k the server sets
 *     x_new = g + tau_eff * sum_k (p_k / a_k) * (x_k - g),        tau_eff = sum_k p_k * a_k,
 * which is FedAvg when all a_k are equal.  The host passes coef[k] = fl32(p_k / a_k) (device
 * float[num_clients]) and tau_eff.  Per coordinate j; every operation is one rounded fp32
 * operation, never fused; denormals are kept:
 *     g   = global[j]
 *     acc = +0.0f
 *     for k = 0 .. num_clients-1, in this order:
 *         x = rows[idx[k]*row_stride + j]                 row_index NULL = identity
 *         d = x - g;   t = coef[k] * d;   acc = acc + t
 *     FH_NOVA_STEP:     s = tau_eff * acc;   out[j] = g + s          the whole rule, one launch
 *     FH_NOVA_PARTIAL:  out[j] = acc          a rank's share of the sum, to all-reduce; global is
 *                                             read, tau_eff is ignored
 *     FH_NOVA_FINISH:   acc = rows[idx[0]*row_stride + j]   rows holds ONE row that IS the
 *                       (all-reduced) sum, coef is not read (may be NULL), num_clients must be 1;
 *                       s = tau_eff * acc;   out[j] = g + s
 * Any NaN result is stored as the one quiet NaN 0x7FC00000.
 * Aliasing: in STEP and FINISH out may be the same pointer as global; in FINISH out may also be
 * the same pointer as rows.  Any other overlap is the caller's error.
 * FH_E_INVALID for: mode outside 0..2; num_clients < 1; FINISH with num_clients != 1; P < 0; a
 * non-finite tau_eff in STEP or FINISH; and, for P > 0, null rows / global / out, or a null coef
 * outside FINISH.  P == 0 is a no-op.  No workspace.  16-byte loads and stores when row_stride % 4
 * == 0 and rows, global and out are 16-byte aligned; a scalar path with the same bits covers
 * everything else and the P % 4 tail.  STEP and PARTIAL read (C+1)*P floats and write P; FINISH
 * reads 2*P and writes P. */
#define FH_NOVA_STEP    0   /* out = g + tau_eff*acc          one launch, one rank      */
#define FH_NOVA_PARTIAL 1   /* out = acc                      a rank's share, to all-reduce */
#define FH_NOVA_FINISH  2   /* rows holds ONE row that IS acc: out = g + tau_eff*acc   */
int fh_fednova_rows(const float* rows, int64_t row_stride, const int32_t* row_index,
                    const float* coef, int32_t num_clients, int64_t P,
                    const float* global, float tau_eff, int32_t mode,
                    float* out, void* stream);

/* ---------------- geometric median and centered clipping (no reference counterpart) --
 * Two robust rules that iterate a weighted sum of the client rows around a centre: the geometric
 * median by the smoothed Weiszfeld iteration (Pillutla, Kakade, Harchaoui, "Robust Aggregation
 * for Federated Learning", IEEE TSP 2022) and centered clipping (Karimireddy, He, Jaggi,
 * "Learning from History for Byzantine Robust Optimization", ICML 2021).  An iteration is one
 * fh_center_iter (the new centre AND every client's squared distance to it, the rows read once)
 * and one fh_center_coef (the next coefficients from those distances).  DESIGN.md §5, D24.
 *
 * fh_center_iter.  x_kj = rows[idx[k]*row_stride + j], row_index NULL = identity; coef: device
 * float[num_clients].  Per coordinate j; every operation is one rounded fp32 operation, never
 * fused; denormals are kept:
 *     acc = +0.0f
 *     for k = 0 .. num_clients-1, in this order, SKIPPING every k whose coef[k] is +0.0f or -0.0f
 *     (its x is not multiplied in: a NaN or Inf row with coefficient 0 cannot reach the sum):
 *         FH_CENTER_MEAN:   t = coef[k] * x_kj;                     acc = acc + t
 *         FH_CENTER_DELTA:  g = center[j];  d = x_kj - g;  t = coef[k] * d;  acc = acc + t
 *     FH_CENTER_MEAN:   out[j] = acc           center is not read and may be NULL
 *     FH_CENTER_DELTA:  out[j] = g + acc       out may be the same pointer as center
 * Any NaN result is stored as the one quiet NaN 0x7FC00000.  In the same pass, for EVERY k
 * (skipped ones included):
 *     sqdist[k] = sum_j ((double)fl32(x_kj - out[j]))^2        out[j] as stored
 * the difference fp32, squares and sums fp64 (the fh_dpfa_row_sqnorm / fh_pairwise_sqdist
 * contract).  sqdist: device double[num_clients].  Each workgroup writes the fp64 partials of its
 * columns to `workspace` (>= fh_center_iter_workspace(num_clients, P) bytes); a second small
 * launch inside the call adds them (per client one wave: lane i adds workgroups i, i+64, ... in
 * order, then a butterfly).  No atomics: the bits of sqdist are a function of num_clients, P and
 * the alignments only, the same on every run.  No allocation, no host synchronisation.
 * Vector loads and stores when row_stride % 4 == 0 and rows, out (and center in DELTA) are
 * 16-byte aligned: 16 bytes per thread for num_clients <= 16, 8 bytes for 17..32 (a thread keeps
 * every client's value of its columns and one fp64 accumulator per client in registers, which
 * sets the width); a scalar path with the same bits of out covers odd strides, misaligned
 * bases, the P % 4 tail and num_clients > 32.  Reads C*P floats (MEAN) or (C+1)*P (DELTA),
 * writes P.
 * FH_E_INVALID for: mode outside 0..1; num_clients outside 1..64; P < 0; null sqdist; and, for
 * P > 0, null rows / coef / out, null center in DELTA, a short or null workspace.  P == 0 is a
 * no-op on out that stores zero distances.  fh_center_iter_workspace is 0 for P <= 0 or
 * num_clients outside 1..64. */
#define FH_CENTER_MEAN  0   /* out = sum_k coef[k]*x_k                (geometric median)  */
#define FH_CENTER_DELTA 1   /* out = center + sum_k coef[k]*(x_k - center)  (centered clip) */
size_t fh_center_iter_workspace(int32_t num_clients, int64_t P);
int fh_center_iter(const float* rows, int64_t row_stride, const int32_t* row_index,
                   const float* coef, int32_t num_clients, int64_t P,
                   const float* center, int32_t mode, float* out,
                   void* workspace, size_t ws_bytes, double* sqdist, void* stream);

/* fh_center_coef: one small launch, all fp64, every operation IEEE-rounded and on its own, sums
 * left to right in k.  sqdist, alpha: device double[num_clients] (alpha: the clients' weights,
 * e.g. n_k / sum n); coef: device float[num_clients]; state: device double[FH_CENTER_STATE_DOUBLES].
 *     d_k    = sqrt(sqdist[k])
 *     live_k = isfinite(sqdist[k]) && alpha[k] > 0
 *   FH_CENTER_GEOMED, param = nu > 0 (the Weiszfeld smoothing):
 *     b_k = live_k ? alpha[k] / max(nu, d_k) : 0;   B = ((b_0 + b_1) + ...)
 *     coef[k] = fl32(b_k / B), all +0 if B == 0
 *   FH_CENTER_CCLIP, param = tau > 0 (the clipping radius):
 *     coef[k] = live_k ? fl32(alpha[k] * (d_k > tau ? tau / d_k : 1.0)) : 0
 *   state[0] = the number of live clients
 *   state[1] = ((o_0 + o_1) + ...), o_k = live_k ? alpha[k] * d_k : 0   (the geometric-median
 *              objective at the centre the distances were taken to)
 *   state[2] = B (GEOMED) or ((coef[0] + coef[1]) + ...) in fp64 (CCLIP)
 *   state[3] = param
 * FH_E_INVALID for: rule outside 0..1; num_clients outside 1..64; a param that is not finite and
 * positive; null pointers. */
#define FH_CENTER_GEOMED 0
#define FH_CENTER_CCLIP  1
#define FH_CENTER_STATE_DOUBLES 4
int fh_center_coef(const double* sqdist, const double* alpha, int32_t num_clients,
                   int32_t rule, double param, float* coef, double* state, void* stream);

/* ---------------- q-FedAvg, fairness-aware aggregation (no reference counterpart) --
 * Li, Sanjabi, Beirami, Smith, "Fair Resource Allocation in Federated Learning" (ICLR 2020),
 * Algorithm 2 with one L cancelled from the numerator and the denominator.  g is the global model
 * the clients started from, x_kj = rows[idx[k]*row_stride + j] (row_index NULL = identity), pi_k
 * the client's weight, F_k >= 0 its loss, q >= 0, L > 0.  The host passes
 *     a[k] = fl32(pi_k * F_k^q)                  device float[num_clients]
 *     b[k] = pi_k * q * L * F_k^(q-1)            device double[num_clients]
 * (fedhip/ops.py qfedavg_coefficients) and the server sets
 *     den   = sum_k ( b[k] * ||x_k - g||^2 + a[k] )
 *     g_new = g + (1/den) * sum_k a[k] * (x_k - g).
 * One call reads the client rows once and keeps den on the device.  DESIGN.md §5, D25.
 *
 * Per coordinate j; every operation is one rounded fp32 operation, never fused; denormals are
 * kept:
 *     g = global[j];  acc = +0.0f
 *     for k = 0 .. num_clients-1, in this order, SKIPPING every k whose a[k] is +0.0f or -0.0f
 *     (its x is not multiplied in: a NaN or Inf row with a[k] = 0 cannot reach the sum):
 *         d = x_kj - g;   t = a[k] * d;   acc = acc + t
 * In the same pass, for EVERY k (skipped ones included):
 *     sqdist[k] = sum_j ((double)fl32(x_kj - g))^2
 * the difference fp32, squares and sums fp64 (the fh_dpfa_row_sqnorm / fh_center_iter contract).
 * sqdist: device double[num_clients].  Each workgroup writes the fp64 partials of its columns to
 * `workspace`; a second small launch adds them (per client one wave: lane i adds workgroups i,
 * i+64, ... in order, then a butterfly) and forms, all fp64, every operation on its own, left to
 * right in k:
 *     live_k = a[k] != 0
 *     h_k    = live_k ? b[k] * sqdist[k] + (double)a[k] : 0
 *     state[0] = den = ((h_0 + h_1) + ...)          state[1] = the number of live clients
 * No atomics: the bits of sqdist and den are a function of num_clients, P and the alignments
 * only, the same on every run.  With
 *     inv = (isfinite(den) && den > 0) ? fl32(1.0 / den) : +0.0f           (fp64 division)
 *   FH_QFA_STEP:     s = inv * acc;   out[j] = g + s.   When inv == 0, out[j] = g bit for bit
 *                    (nothing is multiplied: no 0 * NaN).  acc lives in the workspace between
 *                    the passes; out may be the same pointer as global.
 *   FH_QFA_PARTIAL:  out[j] = acc     a rank's share of the sum, to all-reduce; state[0] is this
 *                    call's share of den, to all-reduce in fp64.  out cannot be global.
 *   FH_QFA_FINISH:   acc = rows[idx[0]*row_stride + j]: rows holds ONE row that IS the
 *                    (all-reduced) sum, num_clients must be 1; state[0] is READ (the all-reduced
 *                    den); out[j] = g + inv * acc as in STEP.  a, b, sqdist may be NULL; no
 *                    workspace; out may be the same pointer as global or as rows.
 * Any NaN result of an arithmetic operation is stored as the one quiet NaN 0x7FC00000.
 * workspace: >= fh_qfedavg_workspace(num_clients, P) bytes, 8-byte aligned (P floats of acc, then
 * the partials).  No allocation, no host synchronisation, a fixed number of launches (at most
 * five).  Vector loads and stores when row_stride % 4 == 0 and rows, global and where acc goes
 * (the workspace in STEP, out in PARTIAL) are 16-byte aligned: 16 bytes per thread for
 * num_clients <= 16, 8 bytes for 17..32 (a thread keeps every client's value of its columns and
 * one fp64 accumulator per client in registers, which sets the width); a scalar path with the
 * same bits of out covers odd strides, misaligned bases, the P % 4 tail and num_clients > 32.
 * The main pass reads (C+1)*P floats and writes P; STEP's second pass reads 2*P and writes P, as
 * does FINISH.
 * FH_E_INVALID for: mode outside 0..2; num_clients outside 1..64 (not exactly 1 in FINISH);
 * P < 0; null state; null a / b / sqdist outside FINISH; and, for P > 0, null rows / global /
 * out, a short, null or misaligned workspace outside FINISH, PARTIAL with out == global.
 * P == 0 stores zero distances and den from the a[k] alone and touches no out.
 * fh_qfedavg_workspace is 0 for P <= 0 or num_clients outside 1..64. */
#define FH_QFA_STEP    0   /* out = g + acc/den              the whole rule, one rank     */
#define FH_QFA_PARTIAL 1   /* out = acc, state[0] = den      a rank's shares, to all-reduce */
#define FH_QFA_FINISH  2   /* rows holds ONE row that IS acc, state[0] IS den: out = g + acc/den */
#define FH_QFA_STATE_DOUBLES 2   /* [0] den, [1] number of live clients */
size_t fh_qfedavg_workspace(int32_t num_clients, int64_t P);
int fh_qfedavg_rows(const float* rows, int64_t row_stride, const int32_t* row_index,
                    const float* a, const double* b, int32_t num_clients, int64_t P,
                    const float* global, int32_t mode, float* out,
                    void* workspace, size_t ws_bytes,
                    double* sqdist, double* state, void* stream);

/* ---------------- FLTrust, trust-scored aggregation (no reference counterpart) --
 * Cao, Fang, Liu, Gong, "FLTrust: Byzantine-robust Federated Learning via Trust Bootstrapping"
 * (NDSS 2021), Algorithm 2.  The server trains on a small clean root shard exactly as a client
 * does; a client's delta is scored by its cosine with the server's delta, negative scores are
 * clipped to zero, every delta is rescaled to the server delta's norm and the scored, rescaled
 * deltas are averaged.  g = global is the vector the round started from, r = root the server's
 * trained row, x_kj = rows[idx[k]*row_stride + j] (row_index NULL = identity), k < num_clients;
 * the root is not one of the clients.  The rule ignores sample counts.  DESIGN.md §5, D26.
 *
 * Every fp32 operation is one rounded operation, never fused; denormals are kept; a NaN result
 * is stored as the one quiet NaN 0x7FC00000 (canon):
 *     d0_j = fl32(r_j - g_j)                 d_kj = fl32(x_kj - g_j)
 *     sq0   = sum_j (double)d0_j^2           sq_k = sum_j (double)d_kj^2
 *     dot_k = sum_j (double)d_kj * (double)d0_j          (every product is exact in fp64)
 * and, in fp64 from here on, every operation IEEE-rounded and on its own, left to right in k:
 *     n0 = sqrt(sq0)      n_k = sqrt(sq_k)
 *     live_k = isfinite(sq_k) && sq_k > 0 && isfinite(dot_k)
 *     q_k  = dot_k / (n_k * n0)
 *     ts_k = live_k ? min(1, max(0, q_k)) : 0            (a NaN q_k gives 0)
 *     S    = ((ts_0 + ts_1) + ...)
 *     c_k  = fl32((ts_k * (n0 / n_k)) / S)   for ts_k > 0;  +0 for ts_k == 0;  all c_k = +0 when
 *            sq0 is not finite or not > 0, or S is not finite or not > 0
 *     acc_j = ((+0 + c_0*d_0j) + c_1*d_1j) + ...   SKIPPING every k with c_k == 0, whatever its
 *                                                  row holds (no 0 * NaN)
 *     out_j = canon(g_j + acc_j);   when every c_k == 0, out = g bit for bit (-0 and NaN payloads
 *                                   of g included)
 * The last two lines are fh_center_iter's FH_CENTER_DELTA arithmetic with center = g, and that is
 * the launch that computes them.
 *
 * One stats pass reads the rows, g and r once ((C+2)*P floats, nothing of size P written) with
 * 2*C + 1 fp64 accumulators per thread; each workgroup writes its partials to the workspace and a
 * one-workgroup launch adds them (per sum one wave: lane i adds workgroups i, i+64, ... in order,
 * then a butterfly) and evaluates the fp64 lines.  33..64 clients take two stats launches over
 * the halves of the index list (g and r are read twice).  No atomics: the bits of every output
 * are a function of num_clients, P and the alignments only.  No allocation, no host
 * synchronisation.  Vector loads when row_stride % 4 == 0 and rows, root and global are 16-byte
 * aligned: 16 bytes per thread for num_clients <= 8, 8 bytes for 9..16; a scalar path with the
 * same kind of sums covers odd strides, misaligned bases, the P % 4 tail and num_clients > 16.
 *   coef:  device float[num_clients], the c_k         trust: device double[num_clients], the ts_k
 *   stats: device double[2*num_clients + 1]: sq_k, then dot_k, then sq0
 *   state: device double[FH_FLT_STATE_DOUBLES]: S, the number of live clients, the number of
 *          clients with ts_k > 0, n0
 *   FH_FLT_SCORE: the two launches above; out is not used and may be NULL.
 *   FH_FLT_STEP:  then out = the new model, by fh_center_iter (DELTA, center = global, these
 *                 coefficients); out may be the same pointer as global.  The first num_clients
 *                 doubles of the workspace then hold every client's squared distance to the new
 *                 model (fh_center_iter's sqdist).
 * workspace: >= fh_fltrust_workspace(num_clients, P) bytes, 8-byte aligned (64 doubles, P floats
 * that keep g for the all-zero case, then the partials of either pass).
 * FH_E_INVALID, with nothing written, for: mode outside 0..1; num_clients outside 1..64; P < 0
 * or row_stride < 0; null coef / trust / stats / state; and, for P > 0, null rows / root /
 * global, null out in STEP, a short, null or misaligned workspace.  P == 0 forms the state from
 * nothing (all sums 0, all coefficients +0) and touches no out and no workspace.
 * fh_fltrust_workspace is 0 for P <= 0 or num_clients outside 1..64. */
#define FH_FLT_SCORE 0   /* coef, trust, stats, state                                  */
#define FH_FLT_STEP  1   /* ... and out = g + sum_k coef[k]*(x_k - g)                  */
#define FH_FLT_STATE_DOUBLES 4   /* [0] S, [1] live clients, [2] clients with ts > 0, [3] n0 */
size_t fh_fltrust_workspace(int32_t num_clients, int64_t P);
int fh_fltrust_rows(const float* rows, int64_t row_stride, const int32_t* row_index,
                    int32_t num_clients, int64_t P, const float* root, const float* global,
                    int32_t mode, float* out, void* workspace, size_t ws_bytes,
                    float* coef, double* trust, double* stats, double* state, void* stream);

/* ---------------- central DP-FedAvg (no reference counterpart) -------------
 * McMahan et al., "Learning Differentially Private Recurrent Language Models" (ICLR 2018): the
 * server clips every client's delta to an L2 norm C_t, averages the clipped deltas with uniform
 * weights 1/m and adds ONE Gaussian draw of standard deviation z*C_t/m; the clip norm follows
 * the target quantile of the clients' norms (Andrew et al., "Differentially Private Learning
 * with Adaptive Clipping", NeurIPS 2021, Alg. 1, geometric update).  DESIGN.md §5 has the
 * definition; x_k = rows[idx[k]*row_stride + .], row_index NULL = identity, g = global.
 *
 * The clip state lives on the device in `state`, FH_DPFA_STATE_DOUBLES doubles:
 *   [FH_DPFA_CLIP]   C_t, the clip norm the next round uses (the caller initialises it)
 *   [FH_DPFA_SIGMA]  sigma_avg of the last fh_dpfa_clip_coef, the fp32 value as a double
 *   [FH_DPFA_BITSUM] this rank's sum of b_k of the last fh_dpfa_clip_coef
 *   [FH_DPFA_BBAR]   bbar of the last fh_dpfa_clip_update
 *   [FH_DPFA_NEXT]   C_{t+1} of the last update (what [FH_DPFA_CLIP] now holds)
 *   [FH_DPFA_PREV]   C_t of the last update (what the last round clipped to)
 * Nothing here allocates or synchronises with the host. */
#define FH_DPFA_STATE_DOUBLES 8
#define FH_DPFA_CLIP   0
#define FH_DPFA_SIGMA  1
#define FH_DPFA_BITSUM 2
#define FH_DPFA_BBAR   3
#define FH_DPFA_NEXT   4
#define FH_DPFA_PREV   5
/* Philox stream words (ctr_hi) of the server's draws: no client id (int64 >= 0) equals them. */
#define FH_DPFA_STREAM_NOISE 0xFFFFFFFFFFFFFFFFull
#define FH_DPFA_STREAM_BIT   0xFFFFFFFFFFFFFFFEull
#define FH_DPFA_ROWS_ARE_DELTAS 1   /* d_k = x_k (global, if given, is only added back) */
#define FH_DPFA_NO_GLOBAL_ADD   2   /* out = the clipped sum [+ noise], without g */

/* sqnorm[k] = sum_j (double)d_kj^2 over the whole row, d_kj = fl32(x_kj - g_j) (global NULL:
 * d = x).  The difference is fp32, squares and sums are fp64.  The summation order is a
 * function of P and of the row's and g's offsets from a 16-byte boundary only: the same input
 * gives the same bits on every run (no atomics).  A (clients, chunks) grid writes fp64 partials
 * to `workspace` (fh_dpfa_row_sqnorm_workspace bytes), a second small launch adds them in
 * order.  16-byte loads where the row and g share their offset from a 16-byte boundary.
 * FH_E_INVALID for num_clients < 1, P < 0, null rows (P > 0) / sqnorm, a short workspace.
 * P == 0 stores zeros. */
size_t fh_dpfa_row_sqnorm_workspace(int32_t num_clients, int64_t P);
int fh_dpfa_row_sqnorm(const float* rows, int64_t row_stride, const int32_t* row_index,
                       const float* global, int32_t num_clients, int64_t P, void* workspace,
                       size_t workspace_bytes, double* sqnorm, void* stream);

/* With C_t = state[FH_DPFA_CLIP], n_k = sqrt(sqnorm[k]) and m = total_clients (the round's
 * clients on ALL ranks; num_clients are this rank's):
 *     bits[k]  = n_k <= C_t
 *     c_k      = n_k > C_t ? fl32(C_t / n_k) : 1.0f       fp64 division; n_k = 0 or NaN: 1
 *     scale[k] = fl32(c_k * fl32(1/m))                    one fp32 multiply
 *     sigma[0] = fl32(z_delta * C_t / m)                  fp64, left to right; sigma may be NULL
 * and state[FH_DPFA_SIGMA], state[FH_DPFA_BITSUM] = sum_k bits[k].  FH_E_INVALID for
 * num_clients < 1, total_clients < num_clients, a negative or non-finite z_delta, null
 * pointers. */
int fh_dpfa_clip_coef(const double* sqnorm, int32_t num_clients, int32_t total_clients,
                      double z_delta, double* state, float* scale, int32_t* bits, float* sigma,
                      void* stream);

/* bbar = (bit_sum[0] + bit_noise * xi) / m;  C_{t+1} = C_t * exp(-clip_lr * (bbar - quantile))
 * in fp64, xi = lane 0 of the fp32 Box-Muller on Philox(seed, FH_DPFA_STREAM_BIT, 0).  With
 * clip_lr == 0: no draw, bbar = bit_sum[0] / m, C_{t+1} = C_t.  bit_sum is a device double
 * (&state[FH_DPFA_BITSUM] on one rank, its all-reduce on several).  Stores BBAR, NEXT, PREV and
 * CLIP = C_{t+1}.  FH_E_INVALID for total_clients < 1, a quantile outside [0, 1], a negative
 * or non-finite clip_lr / bit_noise, null pointers. */
int fh_dpfa_clip_update(double* state, const double* bit_sum, int32_t total_clients,
                        double target_quantile, double clip_lr, double bit_noise, uint64_t seed,
                        void* stream);

/* Per coordinate j, every operation one rounded fp32 operation, never fused:
 *     d_k  = fl32(x_k[j] - g[j])       FH_DPFA_ROWS_ARE_DELTAS or global NULL: d_k = x_k[j]
 *     acc  = (((0 + scale[0]*d_0) + scale[1]*d_1) + ...)              rows in index order
 *     nu   = noise_in ? noise_in[j] : fl32(sigma[0] * G_j)
 *            G_j = lane j%4 of the fp32 Box-Muller on Philox(seed, stream_hi, j/4), as fh_dp_apply's
 *     t    = (noise_in || sigma) ? acc + nu : acc                     no noise: no add
 *     out  = global && !FH_DPFA_NO_GLOBAL_ADD ? g[j] + t : t
 * any NaN is stored as the one quiet NaN 0x7FC00000.  out may alias global or the rows.  With
 * FH_DPFA_ROWS_ARE_DELTAS, one row and scale = {1} on an all-reduced partial the kernel only
 * adds the noise and g.  FH_E_INVALID for num_clients < 1, P < 0, unknown flags, global NULL
 * without FH_DPFA_ROWS_ARE_DELTAS, null rows / scale / out.  P == 0 is a no-op.  16-byte loads
 * and stores when row_stride % 4 == 0 and rows, global, out and noise_in are 16-byte aligned;
 * a scalar kernel with the same bits covers everything else.  Reads (C+1)*P floats, writes P. */
int fh_dpfa_clip_sum(const float* rows, int64_t row_stride, const int32_t* row_index,
                     const float* scale, int32_t num_clients, int64_t P, const float* global,
                     float* out, const float* sigma, const float* noise_in, uint64_t seed,
                     uint64_t stream_hi, int32_t flags, void* stream);

/* ---------------- update-level DP (privacy.py:107-144, 183-254) ----------
 * delta = fl32(local - global) (global may be NULL: delta = local).
 * seg_sqnorm[z*nseg+t] = sum over segment t of delta^2, accumulated in fp64. */
int fh_dp_delta_sqnorm(const float* local, int64_t local_stride, const float* global,
                       int64_t global_stride, int32_t num_clients, const int64_t* seg_offsets,
                       int32_t nseg, double* seg_sqnorm, void* stream);

/* Per client: total = sqrt(sum_t fl32(sqrt(seg_sqnorm_t))^2) (the reference sums
 * squared per-tensor fp32 norms in double, privacy.py:119-123);
 * clipped = total > max_norm; coef = fl32(max_norm/total);
 * sigma = fl32(min(total,max_norm) * sqrt(2 ln(1.25/delta)) / epsilon) (privacy.py:209). */
int fh_dp_clip_coef(const double* seg_sqnorm, int32_t num_clients, int32_t nseg, double max_norm,
                    double epsilon, double delta, double* total_norm, float* coef,
                    int32_t* clipped, float* sigma, void* stream);

/* out = [global +] ( (clipped ? fl32(delta*coef) : delta) + noise ), each step fp32-rounded.
 * noise = noise_in[z*noise_stride + j] if noise_in != NULL (parity mode: noise drawn by
 * the caller) else sigma[z] * N(0,1) from Philox4x32-10 keyed by (seed, z, j). */
int fh_dp_apply(const float* local, int64_t local_stride, const float* global,
                int64_t global_stride, float* out, int64_t out_stride, int32_t num_clients,
                int64_t P, const float* coef, const int32_t* clipped, const float* sigma,
                const float* noise_in, int64_t noise_stride, uint64_t seed,
                const int64_t* row_ids, void* stream);

/* ---------------- optimizers (torch.optim single-tensor semantics) -------- */
/* SGD(momentum, dampening=0, nesterov=False): buf = first ? g : m*buf + g; p -= lr*buf */
int fh_sgd_step(float* param, const float* grad, float* momentum_buf, int64_t n, float lr,
                float momentum, float weight_decay, int32_t first_step, void* stream);
/* Adam / AdamW (decoupled=1). step_size = lr/(1-beta1^t), bc2_sqrt = sqrt(1-beta2^t),
 * both computed by the caller in double exactly as torch.optim does.  scal_dev
 * (nullable): device float[2] = {bc2_sqrt, -step_size} (fp32-rounded) read at run
 * time instead, so one captured step graph serves every step t. */
int fh_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                 double lr, double beta1, double beta2, double eps, double weight_decay,
                 int32_t decoupled, double step_size, double bc2_sqrt, const float* scal_dev,
                 void* stream);

/* Optimizer steps that finish split weight-gradient reductions (r03).  A convolution's
 * weight gradient split over pixel ranges (fh_conv2d_wgrad_deferred) leaves per-split partial
 * sums; the step sums them as its first operation instead of a separate reduction launch.
 * Rows [0, nclients) of param / grad / state at stride row_stride, row_len floats each
 * (row_len and row_stride multiples of 4, rows 16-B aligned).  Inside each slab range
 * [off, off + len) of a row:  g = sum over s of slab[z][s][j - off], summed in the same
 * order and with the same bits as fh_conv2d_wgrad's own reduction, and g is stored to grad;
 * elsewhere g is read from grad.  Then every element gets the fh_sgd_step / fh_adam_step
 * update (same bits).  slabs: HOST array (copied into the launch) of nslabs <=
 * FH_MAX_GRAD_SLABS ranges, sorted, non-overlapping, off and len multiples of 4, each slab
 * 16-B aligned with client stride splits * len.
 * A range with applied != 0 (slab NULL, splits 0) has had its update applied upstream
 * (fh_linear_bwd_fused_upd): the step neither reads nor writes param, grad or state there and
 * spends no workgroup on it.  It still takes part in the sorted / non-overlapping checks.
 * fh_dpsgd_step_slabs refuses such ranges. */
#define FH_MAX_GRAD_SLABS 24
typedef struct {
    int64_t off;       /* first float of the range within a row */
    int64_t len;       /* floats */
    const float* slab; /* device [client][split][len] */
    int32_t splits;
    int32_t applied;   /* != 0: updated upstream, skipped (slab NULL, splits 0) */
} fh_grad_slab;
int fh_sgd_step_slabs(float* param, float* grad, float* momentum_buf, int64_t row_stride,
                      int64_t row_len, int32_t nclients, const fh_grad_slab* slabs,
                      int32_t nslabs, float lr, float momentum, float weight_decay,
                      int32_t first_step, void* stream);
int fh_adam_step_slabs(float* param, float* grad, float* exp_avg, float* exp_avg_sq,
                       int64_t row_stride, int64_t row_len, int32_t nclients,
                       const fh_grad_slab* slabs, int32_t nslabs, double lr, double beta1,
                       double beta2, double eps, double weight_decay, int32_t decoupled,
                       double step_size, double bc2_sqrt, const float* scal_dev, void* stream);

/* DP-SGD step (r04): fh_sgd_step_slabs / fh_adam_step_slabs (adam != 0; decoupled = AdamW)
 * for a per-sample-clipped step.  Each slab range holds one split per IMAGE (splits == batch,
 * fh_conv2d_wgrad_persample's slab): g = sum_{i < counts[z]} coef[z][i] * slab[z][i] in image
 * order; then elements [0, n_noise) of every row get g += (sigma_c / counts[z]) * N(0,1) with
 * fh_dpsgd_noise's Philox keys (seed + *seed_dev, philox_row, the row's float4 index); g is
 * stored and the update applied — the bits of fh_persample_slab_wsum + fh_dpsgd_noise + the
 * optimizer step in one launch.  SGD uses lr / momentum / weight_decay / first_step, Adam lr /
 * beta1 / beta2 / eps / weight_decay / step_size / bc2_sqrt / scal_dev as fh_adam_step. */
/* DP-SGD clip coefficients in one launch (r04): for every (client, image < count) the squared
 * norm of that image's gradient over all layers — linear sources by the rank-1 identity
 * ||dy_i||^2 (||x_i||^2 + with_bias) (x [client][batch][in_f], dy [client][batch][out_f]),
 * slab sources (fh_conv2d_wgrad_persample slabs: weights [client][image][per_w], bias behind
 * them at the 256-B aligned offset) as the sum of squares of the image's rows — in fp64, then
 * coef = min(1, max_norm / (count * sqrt(sum))) (the stored gradients are of the batch-mean
 * loss); images >= count get coef 0.  sqnorm (nullable, fp64 [client][batch]) receives the sums.
 * At most 4 sources of each kind.  Replaces fh_linear_persample_sqnorm / fh_persample_slab_sqnorm
 * per layer + fh_dpsgd_clip_coef. */
typedef struct {
    const float* x;
    int64_t x_cs;
    const float* dy;
    int64_t dy_cs;
    int32_t in_f, out_f, with_bias, reserved;
} fh_linear_norm_src;
typedef struct {
    const void* slab;
    int32_t per_w, per_b;
} fh_slab_norm_src;
int fh_dpsgd_norm_clip(const fh_linear_norm_src* lin, int32_t nlin, const fh_slab_norm_src* slabs,
                       int32_t nslab, const int32_t* counts, int32_t nclients, int32_t batch,
                       double max_norm, double* sqnorm, float* coef, void* stream);
/* fh_conv2d_c1_pool_wgrad_persample + fh_dpsgd_norm_clip in ONE launch (r05): each per-image
 * conv1 slab workgroup ends with the image's norm over the sources (which must include this
 * launch's own slab) and its clip coefficient — fh_dpsgd_norm_clip's code and sums.  cout 32. */
int fh_conv2d_c1_pool_wgrad_persample_clip(
    const float* x, int64_t x_cs, const float* dpool, int64_t dp_cs, const uint8_t* idx,
    int64_t i_cs, const float* y, int64_t y_cs, void* slab, size_t slab_bytes,
    const int32_t* counts, int32_t nclients, int32_t batch, int32_t h, int32_t w, int32_t cout,
    int32_t gh, int32_t gw, const fh_linear_norm_src* lin, int32_t nlin,
    const fh_slab_norm_src* slabs, int32_t nslab, double max_norm, double* sqnorm, float* coef,
    void* stream);
/* fh_linear_wgrad on row-scaled dY: dy row b of client z multiplied by rowscale[z][b] as it is
 * loaded (the products fh_scale_rows would store: same bits as scale_rows + linear_wgrad);
 * DP-SGD's clipped linear-layer sums.  batch <= 32, in_f % 32 == 0. */
int fh_linear_wgrad_rowscale(const float* x, int64_t x_cs, const float* dy, int64_t dy_cs,
                             const float* rowscale, float* dw, int64_t dw_cs, float* db,
                             int64_t db_cs, const int32_t* counts, int32_t nclients,
                             int32_t batch, int32_t in_f, int32_t out_f, void* stream);
/* Up to four linear layers' fh_linear_wgrad_rowscale in ONE launch (the same row scales,
 * counts and batch; each layer's tiles, order and bits as its own call): DP-SGD's pass 2 runs
 * fc2's and fc1's clipped sums as one launch (r05).  batch <= 32, in_f % 32 == 0 per layer. */
typedef struct fh_linear_wgrad_src {
    const float* x;
    int64_t x_cs;
    const float* dy;
    int64_t dy_cs;
    float* dw;
    int64_t dw_cs;
    float* db;      /* nullable */
    int64_t db_cs;
    int32_t in_f, out_f;
} fh_linear_wgrad_src;
int fh_linear_wgrad_rowscale_multi(const fh_linear_wgrad_src* layers, int32_t nlayers,
                                   const float* rowscale, const int32_t* counts,
                                   int32_t nclients, int32_t batch, void* stream);
int fh_dpsgd_step_slabs(float* param, float* grad, float* state1, float* state2,
                        int64_t row_stride, int64_t row_len, int32_t nclients,
                        const fh_grad_slab* slabs, int32_t nslabs, const float* coef,
                        const int32_t* counts, int32_t batch, int64_t n_noise, float sigma_c,
                        uint64_t seed, const uint64_t* seed_dev, int32_t adam, double lr,
                        double momentum, double beta1, double beta2, double eps,
                        double weight_decay, int32_t decoupled, int32_t first_step,
                        double step_size, double bc2_sqrt, const float* scal_dev, void* stream);

/* ---------------- convolution / linear (fp32 MFMA implicit GEMM) ----------
 * x: [clients][batch][cin][h][w]; w: [cout][cin][kh][kw] per client; y: [clients][batch][cout][oh][ow].
 * Supported: (kh,kw,stride) in {(3,3,1),(3,3,2),(1,1,1),(1,1,2)}, pad arbitrary. */
/* FWD/DGRAD split K through `workspace` when the output tiling leaves the chip mostly
 * idle (few clients still training); size it with fh_*_workspace (0 = never splits;
 * a NULL / too-small workspace just disables the split). */
size_t fh_conv2d_fwd_workspace(int32_t nclients, int32_t batch, int32_t cin, int32_t h, int32_t w_,
                               int32_t cout, int32_t kh, int32_t kw, int32_t stride, int32_t pad);
size_t fh_conv2d_dgrad_workspace(int32_t nclients, int32_t batch, int32_t cin, int32_t h,
                                 int32_t w_, int32_t cout, int32_t kh, int32_t kw, int32_t stride,
                                 int32_t pad);
int fh_conv2d_fwd(const float* x, int64_t x_cs, const float* w, int64_t w_cs, const float* bias,
                  int64_t b_cs, float* y, int64_t y_cs, const int32_t* counts, int32_t nclients,
                  int32_t batch, int32_t cin, int32_t h, int32_t w_, int32_t cout, int32_t kh,
                  int32_t kw, int32_t stride, int32_t pad, int32_t relu, void* workspace,
                  size_t ws_bytes, void* stream);
/* accumulate = 1: dx += result (residual-branch gradient sums, ResNet shortcut). */
int fh_conv2d_dgrad(const float* dy, int64_t dy_cs, const float* w, int64_t w_cs, float* dx,
                    int64_t dx_cs, const int32_t* counts, int32_t nclients, int32_t batch,
                    int32_t cin, int32_t h, int32_t w_, int32_t cout, int32_t kh, int32_t kw,
                    int32_t stride, int32_t pad, int32_t accumulate, void* workspace,
                    size_t ws_bytes, void* stream);
/* fh_conv2d_dgrad of a 3x3/s1/p1 conv (direct path: square 8/16/32 maps) whose input was
 * relu(BN(bn_x)): stores g = (bn_x*bn_scale + bn_shift > 0) ? dX : 0 and writes the BN
 * backward partials (sum g, sum (bn_x - bn_mean) g) per (client, channel, 256-pixel tile)
 * to bn_part (fh_conv_bnstats_bytes(nclients, batch, cin, h, w_) bytes) for
 * fh_bn_bwd_tiles.  Replaces the reduce pass of fh_bn_bwd (bn.hip bn_bwd_reduce_kernel);
 * pidx non-NULL: a MaxPool2d(2,2) (+ Dropout: pmask / p_drop, pmask NULL = none) sat
 * between the ReLU and this conv; bn_x is then the 2h x 2w map, dX is stored unmasked and
 * the statistics route it to the window argmax (apply pass: fh_bn_bwd_pool_tiles).
 * reference: CIFAR10CNN conv -> bn -> relu (-> pool -> dropout) -> conv,
 * models_pytorch.py:133-150. */
int fh_conv2d_dgrad_bnstats(const float* dy, int64_t dy_cs, const float* w, int64_t w_cs,
                            float* dx, int64_t dx_cs, const float* bn_x, int64_t bnx_cs,
                            const float* bn_scale, const float* bn_shift, int64_t bns_cs,
                            const float* bn_mean, double* bn_part, const uint8_t* pidx,
                            int64_t pi_cs, const uint8_t* pmask, int64_t pm_cs, float p_drop,
                            const int32_t* counts, int32_t nclients, int32_t batch, int32_t cin,
                            int32_t h, int32_t w_, int32_t cout, void* workspace,
                            size_t ws_bytes, void* stream);
/* dw (and db if non-NULL) are overwritten; the conv-bias gradient is folded into the
 * weight-gradient kernel.  workspace >= fh_conv2d_wgrad_workspace(...) bytes. */
size_t fh_conv2d_wgrad_workspace(int32_t nclients, int32_t batch, int32_t cin, int32_t h,
                                 int32_t w_, int32_t cout, int32_t kh, int32_t kw, int32_t stride,
                                 int32_t pad);
int fh_conv2d_wgrad(const float* x, int64_t x_cs, const float* dy, int64_t dy_cs, float* dw,
                    int64_t dw_cs, float* db, int64_t db_cs, void* workspace, size_t ws_bytes,
                    const int32_t* counts, int32_t nclients, int32_t batch, int32_t cin, int32_t h,
                    int32_t w_, int32_t cout, int32_t kh, int32_t kw, int32_t stride, int32_t pad,
                    void* stream);

/* Linear: x [clients][batch][in_f], w [out_f][in_f], y [clients][batch][out_f]. */
size_t fh_linear_fwd_workspace(int32_t nclients, int32_t batch, int32_t in_f, int32_t out_f);
size_t fh_linear_dgrad_workspace(int32_t nclients, int32_t batch, int32_t in_f, int32_t out_f);
int fh_linear_fwd(const float* x, int64_t x_cs, const float* w, int64_t w_cs, const float* bias,
                  int64_t b_cs, float* y, int64_t y_cs, const int32_t* counts, int32_t nclients,
                  int32_t batch, int32_t in_f, int32_t out_f, int32_t relu, void* workspace,
                  size_t ws_bytes, void* stream);
/* fh_linear_fwd followed by fh_dropout_fwd (F.dropout after the layer's ReLU,
 * models_pytorch.py:153-163) as one product: the dropout runs in the forward epilogue
 * with fh_dropout_fwd's keep-mask draws and element order (drop_mode 1 generate / 2 use
 * mask), so y == dropout_fwd(linear_fwd(x)). */
int fh_linear_fwd_dropout(const float* x, int64_t x_cs, const float* w, int64_t w_cs,
                          const float* bias, int64_t b_cs, float* y, int64_t y_cs, uint8_t* mask,
                          int64_t m_cs, const int32_t* counts, int32_t nclients, int32_t batch,
                          int32_t in_f, int32_t out_f, int32_t relu, int32_t drop_mode,
                          float p_drop, uint64_t seed, const uint64_t* seed_dev, void* workspace,
                          size_t ws_bytes, void* stream);
int fh_linear_dgrad(const float* dy, int64_t dy_cs, const float* w, int64_t w_cs, float* dx,
                    int64_t dx_cs, const int32_t* counts, int32_t nclients, int32_t batch,
                    int32_t in_f, int32_t out_f, void* workspace, size_t ws_bytes, void* stream);
size_t fh_linear_wgrad_workspace(int32_t nclients, int32_t batch, int32_t in_f, int32_t out_f);
int fh_linear_wgrad(const float* x, int64_t x_cs, const float* dy, int64_t dy_cs, float* dw,
                    int64_t dw_cs, float* db, int64_t db_cs, void* workspace, size_t ws_bytes,
                    const int32_t* counts, int32_t nclients, int32_t batch, int32_t in_f,
                    int32_t out_f, void* stream);
/* One launch for a classifier layer's whole backward (nn.Linear.backward + the
 * F.dropout / ReLU backward of its input, models_pytorch.py:153-163): dw, db (nullable) as
 * fh_linear_wgrad, and dx = (dy W) * keep(mask)/(1-p) where relu_ref > 0 (mask, relu_ref
 * nullable: that factor is skipped).  batch <= 32, in_f % 128 == 0, out_f % 32 == 0, dy
 * rows 16-B aligned; FH_E_UNSUPPORTED otherwise. */
int fh_linear_bwd_fused(const float* x, int64_t x_cs, const float* dy, int64_t dy_cs,
                        const float* w, int64_t w_cs, float* dw, int64_t dw_cs, float* db,
                        int64_t db_cs, float* dx, int64_t dx_cs, const uint8_t* mask,
                        int64_t m_cs, float p_drop, const float* relu_ref, int64_t r_cs,
                        const int32_t* counts, int32_t nclients, int32_t batch, int32_t in_f,
                        int32_t out_f, void* stream);

/*
 * fh_linear_bwd_fused_pool: fh_linear_bwd_fused for a layer whose input x is the flattened
 * output of a 2x2 max-pool over ReLU'd maps [C][OH][OW] (SimpleCNN fc1,
 * models_pytorch.py:91-95 — replaces that layer's backward + the pool's fh_maxpool2_bwd):
 * dX is the gradient of the pool INPUT, planes xh x xw (map 2OH x 2OW top-left), the linear
 * dgrad value routed to the window argmax pidx (dense [C][OH][OW]) where x > 0, zeros at the
 * other window positions; elements outside the map untouched.
 */
int fh_linear_bwd_fused_pool(const float* x, int64_t x_cs, const float* dy, int64_t dy_cs,
                             const float* w, int64_t w_cs, float* dw, int64_t dw_cs, float* db,
                             int64_t db_cs, float* dx, int64_t dx_cs, const uint8_t* pidx,
                             int64_t pi_cs, const int32_t* counts, int32_t nclients, int32_t batch,
                             int32_t C, int32_t OH, int32_t OW, int32_t xh, int32_t xw,
                             int32_t out_f, void* stream);

/*
 * The fused linear backward with the optimizer update applied where the weight gradient is
 * produced (fh_linear_bwd_fused_upd, fh_linear_bwd_fused_pool_upd).  When the update is fused,
 * the layer's DGRAD is launched first (it reads the weights) and the WGRAD launch then applies
 * fh_sgd_step's / fh_adam_step's update to the layer's weight and bias elements instead of
 * storing dw / db: same gradient bits, same update operations, so parameters and state equal
 * the unfused call followed by fh_sgd_step_slabs / fh_adam_step_slabs bit for bit; dw and db
 * are then left untouched and the optimizer launch must skip their ranges (fh_grad_slab.applied).
 * *applied (required) says which happened: 1 = the update is applied, 0 = the launch was
 * fh_linear_bwd_fused's own (dw / db written, parameters untouched).
 *   mode 1: fuse only at the widths where the backward already runs as two launches;
 *   mode 2: fuse at every width (two launches where one dual-role launch ran before).
 * pw / pb: the layer's weight / bias in the parameter rows (pw is normally w itself); s1* / s2*:
 * the same elements of the optimizer state rows, at the parameters' client strides (s1 NULL
 * for SGD without momentum, s2 used by Adam only).  The scalars are those of fh_sgd_step
 * (adam == 0: lr, momentum, weight_decay, first_step) or fh_adam_step (adam != 0), scal_dev
 * included.  pb and the bias states may be NULL when db is NULL.
 */
typedef struct {
    float* pw;
    int64_t pw_cs;
    float* pb;
    int64_t pb_cs;
    float* s1w;
    float* s1b;
    float* s2w;
    float* s2b;
    int32_t adam, decoupled, first_step, mode;
    double lr, momentum, weight_decay, beta1, beta2, eps, step_size, bc2_sqrt;
    const float* scal_dev;
} fh_linear_update;
int fh_linear_bwd_fused_upd(const float* x, int64_t x_cs, const float* dy, int64_t dy_cs,
                            const float* w, int64_t w_cs, float* dw, int64_t dw_cs, float* db,
                            int64_t db_cs, float* dx, int64_t dx_cs, const uint8_t* mask,
                            int64_t m_cs, float p_drop, const float* relu_ref, int64_t r_cs,
                            const int32_t* counts, int32_t nclients, int32_t batch,
                            int32_t in_f, int32_t out_f, const fh_linear_update* upd,
                            int32_t* applied, void* stream);
int fh_linear_bwd_fused_pool_upd(const float* x, int64_t x_cs, const float* dy, int64_t dy_cs,
                                 const float* w, int64_t w_cs, float* dw, int64_t dw_cs,
                                 float* db, int64_t db_cs, float* dx, int64_t dx_cs,
                                 const uint8_t* pidx, int64_t pi_cs, const int32_t* counts,
                                 int32_t nclients, int32_t batch, int32_t C, int32_t OH,
                                 int32_t OW, int32_t xh, int32_t xw, int32_t out_f,
                                 const fh_linear_update* upd, int32_t* applied, void* stream);

/* ---------------- BatchNorm2d (+ReLU, +residual add) ----------------------
 * x/y/res: [clients][batch][C][HW]; gamma/beta live in the per-client param
 * rows (stride p_cs); running stats stride r_cs (NULL: not tracked);
 * save_mean/save_invstd: [clients][C].  Train mode: batch statistics over the
 * valid images (fp64 accumulation), running stats momentum-updated with the
 * unbiased variance.  y = relu?( x*alpha + beta' [+ res] ).
 * Each (client, channel) reduction is split over several workgroups; their
 * partials go to `workspace` (>= fh_bn_workspace bytes, shared by train fwd
 * and bwd) and are merged in a fixed order: results are deterministic. */
size_t fh_bn_workspace(int32_t nclients, int32_t batch, int32_t C, int32_t HW);
int fh_bn_fwd_train(const float* x, int64_t x_cs, float* y, int64_t y_cs, const float* res,
                    int64_t res_cs, const float* gamma, const float* beta, int64_t p_cs,
                    float* running_mean, float* running_var, int64_t r_cs, float* save_mean,
                    float* save_invstd, const int32_t* counts, int32_t nclients, int32_t batch,
                    int32_t C, int32_t HW, float eps, float momentum, int32_t relu,
                    void* workspace, size_t ws_bytes, void* stream);
int fh_bn_fwd_eval(const float* x, int64_t x_cs, float* y, int64_t y_cs, const float* res,
                   int64_t res_cs, const float* gamma, const float* beta, int64_t p_cs,
                   const float* running_mean, const float* running_var, int64_t r_cs,
                   const int32_t* counts, int32_t nclients, int32_t batch, int32_t C, int32_t HW,
                   float eps, int32_t relu, void* stream);
/* g = relu ? dy*(yout>0) : dy; dres (nullable) <- g; dgamma/dbeta (stride g_cs) and dx.
 * With relu and yout NULL the mask is recomputed from x (x*alpha + beta' > 0, the
 * forward's own fp32 operations; needs beta, and no residual add before the ReLU). */
int fh_bn_bwd(const float* dy, int64_t dy_cs, const float* yout, int64_t yo_cs, const float* x,
              int64_t x_cs, const float* gamma, const float* beta, int64_t p_cs,
              const float* save_mean,
              const float* save_invstd, float* dx, int64_t dx_cs, float* dres, int64_t dres_cs,
              float* dgamma, float* dbeta, int64_t g_cs, const int32_t* counts, int32_t nclients,
              int32_t batch, int32_t C, int32_t HW, int32_t relu, void* workspace,
              size_t ws_bytes, void* stream);

/* BN backward apply from the partials fh_conv2d_dgrad_bnstats left (g already masked):
 * dgamma / dbeta (stride dg_cs) and dx, as fh_bn_bwd's second pass. */
int fh_bn_bwd_tiles(const double* part, const float* g, int64_t g_cs, const float* x,
                    int64_t x_cs, const float* gamma, int64_t p_cs, const float* save_mean,
                    const float* save_invstd, float* dx, int64_t dx_cs, float* dgamma,
                    float* dbeta, int64_t dg_cs, const int32_t* counts, int32_t nclients,
                    int32_t batch, int32_t C, int32_t HW, void* stream);

/* fh_bn_bwd_pool's apply pass from the partials fh_conv2d_dgrad_bnstats(pidx != NULL)
 * left: dgamma / dbeta and dx (H x W: the BN's map), ReLU mask recomputed from x. */
int fh_bn_bwd_pool_tiles(const double* part, const float* dpool, int64_t dp_cs,
                         const uint8_t* pidx, int64_t pi_cs, const uint8_t* pmask, int64_t pm_cs,
                         float p_drop, const float* x, int64_t x_cs, const float* gamma,
                         const float* beta, int64_t p_cs, const float* save_mean,
                         const float* save_invstd, float* dx, int64_t dx_cs, float* dgamma,
                         float* dbeta, int64_t g_cs, const int32_t* counts, int32_t nclients,
                         int32_t batch, int32_t C, int32_t H, int32_t W, void* stream);

/* BN backward whose upstream gradient comes through MaxPool2d(2,2) (+ the Dropout
 * fused after it, p_drop / pmask as in fh_maxpool2_fwd; pmask NULL = no dropout):
 * the full-resolution gradient is routed from dpool [clients][batch][C][H/2][W/2]
 * by the argmax bytes pidx on the fly (fh_maxpool2_bwd + fh_bn_bwd in one pass pair). */
int fh_bn_bwd_pool(const float* dpool, int64_t dp_cs, const uint8_t* pidx, int64_t pi_cs,
                   const uint8_t* pmask, int64_t pm_cs, float p_drop, const float* yout,
                   int64_t yo_cs, const float* x, int64_t x_cs, const float* gamma,
                   const float* beta, int64_t p_cs, const float* save_mean, const float* save_invstd, float* dx, int64_t dx_cs,
                   float* dgamma, float* dbeta, int64_t g_cs, const int32_t* counts,
                   int32_t nclients, int32_t batch, int32_t C, int32_t H, int32_t W, int32_t relu,
                   void* workspace, size_t ws_bytes, void* stream);

/* ---------------- DP-SGD: per-sample clipping (north_star extension) -------
 * g = (sum_i min(1, C/||g_i||) g_i + sigma*C*N(0,I)) / B per optimizer step, g_i the
 * gradient of sample i's loss over ALL parameters.  The caller accumulates
 * ||g_i/B||^2 layer by layer into sqnorm [clients][batch] (double; zero it first):
 *   convs   fh_conv2d_persample_sqnorm (per-image WGRAD tiles, workspace query below)
 *   linears fh_linear_persample_sqnorm (||dy_i||^2 (||x_i||^2 + with_bias))
 * then fh_dpsgd_clip_coef -> coef [clients][batch], fh_scale_rows scales each layer's
 * upstream gradient rows by coef before the ordinary WGRAD (clipped sum), and
 * fh_dpsgd_noise adds sigma*C/B * N(0,1) (Philox key seed + seed_dev[0], rows keyed as below).
 * Replaces: nothing in the reference (its DP clips whole update deltas, privacy.py:107-144);
 * sigma follows its Gaussian-mechanism formula (privacy.py:209). */
size_t fh_conv2d_persample_sqnorm_workspace(int32_t nclients, int32_t batch, int32_t cin,
                                            int32_t h, int32_t w, int32_t cout, int32_t kh,
                                            int32_t kw, int32_t stride, int32_t pad);
int fh_conv2d_persample_sqnorm(const float* x, int64_t x_cs, const float* dy, int64_t dy_cs,
                               int32_t with_bias, double* sqnorm, void* workspace,
                               size_t ws_bytes, const int32_t* counts, int32_t nclients,
                               int32_t batch, int32_t cin, int32_t h, int32_t w, int32_t cout,
                               int32_t kh, int32_t kw, int32_t stride, int32_t pad, void* stream);
int fh_linear_persample_sqnorm(const float* x, int64_t x_cs, const float* dy, int64_t dy_cs,
                               int32_t with_bias, double* sqnorm, const int32_t* counts,
                               int32_t nclients, int32_t batch, int32_t in_f, int32_t out_f,
                               void* stream);
/* DP-SGD on the direct kernels (r04): per-image weight-gradient slabs.  A direct WGRAD with one
 * pixel split per image leaves slab [client][image][cout*cin*9] (the gradient of that image's
 * share of the batch-mean loss, g_i / B) and the bias slab [client][image][cout] behind it at a
 * 256-B aligned offset; fh_conv2d_wgrad_persample_workspace gives the slab bytes.
 * fh_conv2d_wgrad_persample: 3x3/s1/p1 on square 8/16/32 maps, channels % 32 (SimpleCNN conv2
 * on its padded 16x16 planes).  fh_conv2d_c1_pool_wgrad_persample: the single-input-channel
 * conv1 from pool1's gradient (fh_conv2d_c1_pool_wgrad's routing), h % 4 == 0.
 * fh_persample_slab_sqnorm: sqnorm[client][image] (fp64, [nclients][batch]) += the image's sum
 * of squares over the slab (weights + bias; per_w % 4 == 0).  fh_persample_slab_wsum: dw =
 * sum_{i < count} coef[client][i] * slab[client][i] in image order (fp32 multiply then add),
 * db likewise from the bias slab (per_b = 0: no bias).  Together they replace the per-sample
 * norm pass and the second WGRAD on coefficient-scaled rows (reference: per-sample clipping is
 * not in the reference; its update clip is privacy.py:107-144, sigma privacy.py:209). */
size_t fh_conv2d_wgrad_persample_workspace(int32_t nclients, int32_t batch, int32_t cin,
                                           int32_t cout);
int fh_conv2d_wgrad_persample(const float* x, int64_t x_cs, const float* dy, int64_t dy_cs,
                              void* slab, size_t slab_bytes, const int32_t* counts,
                              int32_t nclients, int32_t batch, int32_t cin, int32_t h, int32_t w,
                              int32_t cout, void* stream);
int fh_conv2d_c1_pool_wgrad_persample(const float* x, int64_t x_cs, const float* dpool,
                                      int64_t dp_cs, const uint8_t* idx, int64_t i_cs,
                                      const float* y, int64_t y_cs, void* slab, size_t slab_bytes,
                                      const int32_t* counts, int32_t nclients, int32_t batch,
                                      int32_t h, int32_t w, int32_t cout, int32_t gh, int32_t gw,
                                      void* stream);
int fh_persample_slab_sqnorm(const void* slab, int32_t per_w, int32_t per_b,
                             const int32_t* counts, int32_t nclients, int32_t batch,
                             double* sqnorm, void* stream);
int fh_persample_slab_wsum(const void* slab, int32_t per_w, int32_t per_b, const float* coef,
                           const int32_t* counts, int32_t nclients, int32_t batch, float* dw,
                           int64_t dw_cs, float* db, int64_t db_cs, void* stream);
int fh_dpsgd_clip_coef(const double* sqnorm, const int32_t* counts, int32_t nclients,
                       int32_t batch, double max_norm, float* coef, void* stream);
int fh_scale_rows(const float* in, int64_t in_cs, const float* coef, const int32_t* counts,
                  int32_t nclients, int32_t batch, int64_t per_img, float* out, int64_t out_cs,
                  void* stream);
int fh_dpsgd_noise(float* grad, int64_t g_cs, int64_t n, const int32_t* counts, int32_t nclients,
                   int32_t batch, float sigma_c, uint64_t seed, const uint64_t* seed_dev,
                   void* stream);

/* ---------------- MaxPool2d(2,2) (+ fused Dropout after it) ---------------
 * idx: uint8 window argmax [clients][batch][C][H/2][W/2]; drop_mode 0 none,
 * 1 generate keep-mask (Philox4x32-10 keyed by seed, slot, element) into mask,
 * 2 apply the caller's mask (parity).  The Philox key is seed + seed_dev[0]
 * (seed_dev nullable: a per-step device key block for graph replay).  Every seed_dev of
 * this header points to that block, {step key, n_ids, id[0..n_ids)} (uint64): with
 * n_ids != 0 client row z draws under id[z] (its global client id) instead of z, so a
 * client's dropout / augmentation / DP-SGD noise does not depend on its slot.
 * Backward writes all four window slots;
 * xin (nullable) = the pooled ReLU output, to apply the ReLU mask at the argmax. */
int fh_maxpool2_fwd(const float* x, int64_t x_cs, float* y, int64_t y_cs, uint8_t* idx,
                    int64_t i_cs, uint8_t* mask, int64_t m_cs, const int32_t* counts,
                    int32_t nclients, int32_t batch, int32_t C, int32_t H, int32_t W,
                    int32_t drop_mode, float p_drop, uint64_t seed, const uint64_t* seed_dev,
                    void* stream);
int fh_maxpool2_bwd(const float* dy, int64_t dy_cs, const uint8_t* idx, int64_t i_cs,
                    const uint8_t* mask, int64_t m_cs, float p_drop, const float* xin, int64_t x_cs,
                    float* dx, int64_t dx_cs, const int32_t* counts, int32_t nclients,
                    int32_t batch, int32_t C, int32_t H, int32_t W, void* stream);
/* The same pools on H x W maps embedded in the top-left corner of larger planes (SimpleCNN's
 * 14x14 conv runs on 16x16 planes with a zero ring on the direct-conv path): fwd x planes
 * xh x xw and y planes yh x yw; bwd dy planes gh x gw, dx / xin planes xh x xw; idx / mask
 * stay dense [img][C][H/2][W/2].  Nothing outside the map is written. */
int fh_maxpool2_fwd_pitched(const float* x, int64_t x_cs, float* y, int64_t y_cs, uint8_t* idx,
                            int64_t i_cs, uint8_t* mask, int64_t m_cs, const int32_t* counts,
                            int32_t nclients, int32_t batch, int32_t C, int32_t H, int32_t W,
                            int32_t drop_mode, float p_drop, uint64_t seed,
                            const uint64_t* seed_dev, int32_t xh, int32_t xw, int32_t yh,
                            int32_t yw, void* stream);
int fh_maxpool2_bwd_pitched(const float* dy, int64_t dy_cs, const uint8_t* idx, int64_t i_cs,
                            const uint8_t* mask, int64_t m_cs, float p_drop, const float* xin,
                            int64_t x_cs, float* dx, int64_t dx_cs, const int32_t* counts,
                            int32_t nclients, int32_t batch, int32_t C, int32_t H, int32_t W,
                            int32_t gh, int32_t gw, int32_t xh, int32_t xw, void* stream);

/* ---------------- Dropout (F.dropout: x * bernoulli(1-p)/(1-p)) ------------
 * drop_mode 1 generate mask (uint8), 2 use the caller's mask.  Backward:
 * dx = dy*mask/(1-p) [* (relu_out > 0)]; mask NULL = ReLU backward only. */
int fh_dropout_fwd(const float* x, int64_t x_cs, float* y, int64_t y_cs, uint8_t* mask,
                   int64_t m_cs, const int32_t* counts, int32_t nclients, int32_t batch,
                   int64_t per_img, int32_t drop_mode, float p_drop, uint64_t seed,
                   const uint64_t* seed_dev, void* stream);
int fh_dropout_bwd(const float* dy, int64_t dy_cs, const uint8_t* mask, int64_t m_cs, float p_drop,
                   const float* relu_out, int64_t r_cs, float* dx, int64_t dx_cs,
                   const int32_t* counts, int32_t nclients, int32_t batch, int64_t per_img,
                   void* stream);

/* ---------------- CrossEntropyLoss (mean) fwd+bwd + epoch metrics ---------
 * targets int64 [clients][batch]; dlogits = (softmax - onehot)/count;
 * loss_out[z] = batch mean loss; acc_* (nullable) accumulate the epoch's
 * sum of batch losses, correct argmax predictions and samples seen;
 * reset[z] != 0 (nullable) restarts client z's accumulators (epoch boundary). */
int fh_ce_fwd_bwd(const float* logits, int64_t l_cs, const int64_t* targets, int64_t t_cs,
                  float* dlogits, int64_t d_cs, float* loss_out, double* acc_loss,
                  int64_t* acc_correct, int64_t* acc_seen, const int32_t* reset,
                  const int32_t* counts, int32_t nclients, int32_t batch, int32_t num_classes,
                  void* stream);
/* The classifier head of a training step in one launch per client (replaces the last
 * nn.Linear forward, fh_ce_fwd_bwd, that layer's wgrad / dgrad and the dropout backward in
 * front of it: CIFAR10CNN fc3 models_pytorch.py:159-165, SimpleCNN fc2 :96-97,
 * FederatedResNet fc :241-246, with LocalTrainer's criterion training.py:193-203):
 * logits = x W^T + b (also stored), CE outputs exactly as fh_ce_fwd_bwd, dw / db (nullable),
 * and dx (nullable) = (dlogits W) * keep(mask)/(1-p), zeroed where relu_in and x <= 0.
 * batch <= 32, num_classes <= 128. */
int fh_linear_head_ce(const float* x, int64_t x_cs, const float* w, int64_t w_cs,
                      const float* bias, int64_t b_cs, const int64_t* targets, int64_t t_cs,
                      float* logits, int64_t l_cs, float* dlogits, int64_t d_cs, float* loss_out,
                      double* acc_loss, int64_t* acc_correct, int64_t* acc_seen,
                      const int32_t* reset, float* dw, int64_t dw_cs, float* db, int64_t db_cs,
                      float* dx, int64_t dx_cs, const uint8_t* mask, int64_t m_cs, float p_drop,
                      int32_t relu_in, const int32_t* counts, int32_t nclients, int32_t batch,
                      int32_t in_f, int32_t num_classes, void* stream);

/* ---------------- BatchNorm apply + ReLU folded into the consumer (CIFAR10CNN) -------
 * The train-mode BN output relu(x*w*invstd + b - mean*w*invstd) is never written: the
 * statistics pass ends in a per-(client, channel) affine (scale, shift [z][C], stride
 * s_cs) and every consumer of the activation — the next conv's forward and weight
 * gradient, or the 2x2 max-pool — applies relu(x*scale + shift) while loading x.
 * Same fp32 operations as fh_bn_fwd_train's apply pass, so results are bit-identical.
 * (models_pytorch.py:128-137: conv -> bn -> relu -> conv / pool.) */
int fh_bn_fwd_stats(const float* x, int64_t x_cs, const float* gamma, const float* beta,
                    int64_t p_cs, float* running_mean, float* running_var, int64_t r_cs,
                    float* save_mean, float* save_invstd, float* scale_out, float* shift_out,
                    int64_t s_cs, const int32_t* counts, int32_t nclients, int32_t batch,
                    int32_t C, int32_t HW, float eps, float momentum, void* workspace,
                    size_t ws_bytes, void* stream);
/* fh_conv2d_fwd / fh_conv2d_wgrad with x = a BN pre-activation (direct 3x3 path only:
 * 3x3/s1/p1 on 8/16/32 square maps; wgrad also needs cin, cout % 32 == 0; else
 * FH_E_UNSUPPORTED).  Zero padding is applied after the affine (padding of the ReLU
 * output, as in the reference). */
int fh_conv2d_fwd_bnrelu(const float* x, int64_t x_cs, const float* in_scale,
                         const float* in_shift, int64_t aff_cs, const float* w, int64_t w_cs,
                         const float* bias, int64_t b_cs, float* y, int64_t y_cs,
                         const int32_t* counts, int32_t nclients, int32_t batch, int32_t cin,
                         int32_t h, int32_t w_, int32_t cout, int32_t kh, int32_t kw,
                         int32_t stride, int32_t pad, int32_t relu, void* workspace,
                         size_t ws_bytes, void* stream);
int fh_conv2d_wgrad_bnrelu(const float* x, int64_t x_cs, const float* in_scale,
                           const float* in_shift, int64_t aff_cs, const float* dy, int64_t dy_cs,
                           float* dw, int64_t dw_cs, float* db, int64_t db_cs, void* workspace,
                           size_t ws_bytes, const int32_t* counts, int32_t nclients,
                           int32_t batch, int32_t cin, int32_t h, int32_t w_, int32_t cout,
                           int32_t kh, int32_t kw, int32_t stride, int32_t pad, void* stream);
/* fh_conv2d_wgrad (in_scale / in_shift NULL) or fh_conv2d_wgrad_bnrelu without the final
 * reduction: when the kernel leaves partial sums (*splits_out >= 1 of them) they stay in `slab`
 * (sized by fh_conv2d_wgrad_workspace) — weights [client][split][cout*cin*kh*kw] at byte 0,
 * bias [client][split][cout] at byte *bias_off_out — for an optimizer step to finish
 * (fh_sgd_step_slabs / fh_adam_step_slabs; a one-split slab is copied by it);
 * *splits_out == 0: dw / db written directly.  (r06: one-split slab plans — single-channel,
 * small-cin and stride-2 kernels — used to report 1, read as "written directly", so that
 * layer's gradient was dropped; found by tests/test_full_plan_resnet_gpu.py, K5.) */
int fh_conv2d_wgrad_deferred(const float* x, int64_t x_cs, const float* in_scale,
                             const float* in_shift, int64_t aff_cs, const float* dy,
                             int64_t dy_cs, float* dw, int64_t dw_cs, float* db, int64_t db_cs,
                             void* slab, size_t slab_bytes, const int32_t* counts,
                             int32_t nclients, int32_t batch, int32_t cin, int32_t h, int32_t w_,
                             int32_t cout, int32_t kh, int32_t kw, int32_t stride, int32_t pad,
                             int32_t* splits_out, int64_t* bias_off_out, void* stream);
int fh_maxpool2_fwd_bnrelu(const float* x, int64_t x_cs, const float* in_scale,
                           const float* in_shift, int64_t aff_cs, float* y, int64_t y_cs,
                           uint8_t* idx, int64_t i_cs, uint8_t* mask, int64_t m_cs,
                           const int32_t* counts, int32_t nclients, int32_t batch, int32_t C,
                           int32_t H, int32_t W, int32_t drop_mode, float p_drop, uint64_t seed,
                           const uint64_t* seed_dev, void* stream);
/* BatchNorm statistics from the producing convolution (models_pytorch.py:128-137 conv ->
 * bn; replaces the statistics pass of nn.BatchNorm2d's train forward): the direct-conv
 * forward (fh_conv2d_fwd_bnrelu semantics, in_scale/in_shift nullable, no ReLU on y) also
 * writes one fp64 (sum of y, sum of y^2) pair per (client, channel, 256-pixel tile of the
 * client's [batch*H*W] pixels) into bn_part (fh_conv_bnstats_bytes; tiles past a client's
 * count are zero), and fh_bn_finalize_tiles merges them in tile order into fh_bn_fwd_stats'
 * outputs — y is never re-read for its statistics. */
size_t fh_conv_bnstats_bytes(int32_t nclients, int32_t batch, int32_t cout, int32_t h,
                             int32_t w_);
int fh_conv2d_fwd_bnstats(const float* x, int64_t x_cs, const float* in_scale,
                          const float* in_shift, int64_t aff_cs, const float* w, int64_t w_cs,
                          const float* bias, int64_t b_cs, float* y, int64_t y_cs,
                          double* bn_part, const int32_t* counts, int32_t nclients,
                          int32_t batch, int32_t cin, int32_t h, int32_t w_, int32_t cout,
                          void* workspace, size_t ws_bytes, void* stream);
/* conv (3x3 / s1 / p1, bias) -> ReLU -> 2x2 max-pool of the top-left pool_hw x pool_hw map of
 * each h x w plane (h = w = 8 or 16): SimpleCNN conv2 -> relu -> pool2 on the 16x16 planes that
 * hold its 14x14 map (replaces conv2d_fwd + maxpool2_fwd of models_pytorch.py:88-89).  py /
 * pidx: dense [img][cout][pool_hw/2][pool_hw/2], the values and first-max argmax of
 * fh_maxpool2_fwd_pitched bit for bit: pooled in the conv's epilogue (unsplit launches) or in
 * the split-K reduction (16x16 planes).  y (h x w planes) is scratch, written only by split
 * launches on 8x8 planes (pooled by a separate pass); the pool's backward takes its ReLU mask
 * from py (fh_maxpool2_bwd_ymask). */
int fh_conv2d_fwd_relu_pool(const float* x, int64_t x_cs, const float* w, int64_t w_cs,
                            const float* bias, int64_t b_cs, float* y, int64_t y_cs, float* py,
                            int64_t py_cs, uint8_t* pidx, int64_t pi_cs, const int32_t* counts,
                            int32_t nclients, int32_t batch, int32_t cin, int32_t h, int32_t w_,
                            int32_t cout, int32_t pool_hw, void* workspace, size_t ws_bytes,
                            void* stream);
/* fh_bn_finalize_tiles fused into the 2x2 max-pool (+dropout, drop_mode as fh_maxpool2_fwd)
 * of the BN-ReLU output (CIFAR10CNN conv -> bn -> relu -> pool -> dropout,
 * models_pytorch.py:139-155): the same outputs as fh_bn_finalize_tiles followed by
 * fh_maxpool2_fwd_bnrelu, one launch. */
int fh_maxpool2_fwd_bnfinalize(const double* part, const float* gamma, const float* beta,
                               int64_t p_cs, float* running_mean, float* running_var,
                               int64_t r_cs, float* save_mean, float* save_invstd,
                               float* scale_out, float* shift_out, int64_t s_cs, const float* x,
                               int64_t x_cs, float* y, int64_t y_cs, uint8_t* idx, int64_t i_cs,
                               uint8_t* mask, int64_t m_cs, const int32_t* counts,
                               int32_t nclients, int32_t batch, int32_t C, int32_t H, int32_t W,
                               float eps, float momentum, int32_t drop_mode, float p_drop,
                               uint64_t seed, const uint64_t* seed_dev, void* stream);
int fh_bn_finalize_tiles(const double* part, const float* gamma, const float* beta,
                         int64_t p_cs, float* running_mean, float* running_var, int64_t r_cs,
                         float* save_mean, float* save_invstd, float* scale_out,
                         float* shift_out, int64_t s_cs, const int32_t* counts,
                         int32_t nclients, int32_t batch, int32_t C, int32_t HW, float eps,
                         float momentum, void* stream);
/* The input gradient of a ResNet down-sampling block in one launch (models_pytorch.py:176-194:
 * conv1 3x3/s2/p1 and the 1x1/s2 projection shortcut read the same input):
 * dx (=|+=) dgrad_3x3s2(dy, w) + dgrad_1x1s2(dy_sc, w_sc); dy_sc has dy's shape, w_sc is
 * [cout][cin] per client.  Replaces the two fh_conv2d_dgrad calls (the second accumulating).
 * Direct stride-2 kernel only (square 32/16 maps, cin % 32 == 0, cout % 8 == 0, aligned
 * rows): FH_E_UNSUPPORTED otherwise.  Workspace: fh_conv2d_dgrad_workspace of the 3x3. */
int fh_conv2d_dgrad_s2_shortcut(const float* dy, int64_t dy_cs, const float* w, int64_t w_cs,
                                const float* dy_sc, int64_t dysc_cs, const float* w_sc,
                                int64_t wsc_cs, float* dx, int64_t dx_cs, const int32_t* counts,
                                int32_t nclients, int32_t batch, int32_t cin, int32_t h, int32_t w_,
                                int32_t cout, int32_t accumulate, void* workspace, size_t ws_bytes,
                                void* stream);
/* SimpleCNN conv1 -> ReLU -> 2x2 max-pool (models_pytorch.py:80-82) in one launch: cin = 1,
 * 3x3/s1/p1, cout 32 or 64; y = the pooled output in planes yh x yw (map in the top-left
 * corner), idx the dense uint8 window argmax; the same values as fh_conv2d_fwd(relu=1) +
 * fh_maxpool2_fwd, the full-resolution ReLU output never written. */
int fh_conv2d_c1_pool_fwd(const float* x, int64_t x_cs, const float* w, int64_t w_cs,
                          const float* bias, int64_t b_cs, float* y, int64_t y_cs, uint8_t* idx,
                          int64_t i_cs, const int32_t* counts, int32_t nclients, int32_t batch,
                          int32_t h, int32_t w_, int32_t cout, int32_t yh, int32_t yw,
                          void* stream);
/* fh_conv2d_c1_pool_fwd with the step's batch gather folded in (r04): x [client][batch][h][w]
 * is WRITTEN from the raw uint8 images data[gidx[client][b]] ([N][h][w], one channel) with
 * fh_gather_u8's normalisation (x = (u / 255 - mean) / std; no crop / flip) and
 * y_lab[client][b] = labels[gidx[client][b]] — fh_gather_u8's x and labels bit for bit — and
 * the pooled output / argmax as fh_conv2d_c1_pool_fwd on that x.  Replaces gather +
 * conv1 -> relu -> pool1 of SimpleCNN's training step (data_loader.py:298-301,
 * models_pytorch.py:86-87). */
int fh_conv2d_c1_pool_fwd_u8(const uint8_t* data, const int64_t* labels, const int64_t* gidx,
                             int64_t g_cs, float mean, float stdv, float* x, int64_t x_cs,
                             int64_t* y_lab, int64_t yl_cs, const float* w, int64_t w_cs,
                             const float* bias, int64_t b_cs, float* y, int64_t y_cs,
                             uint8_t* idx, int64_t i_cs, const int32_t* counts, int32_t nclients,
                             int32_t batch, int32_t h, int32_t w_, int32_t cout, int32_t yh,
                             int32_t yw, void* stream);
/* fh_maxpool2_bwd (pitched planes: dy / y gh x gw, dx xh x xw) with the ReLU mask at the
 * argmax taken from the pooled output y (> 0), for a forward that never wrote the
 * full-resolution ReLU output (fh_conv2d_c1_pool_fwd); no dropout. */
int fh_maxpool2_bwd_ymask(const float* dy, int64_t dy_cs, const uint8_t* idx, int64_t i_cs,
                          const float* y, int64_t y_cs, float* dx, int64_t dx_cs,
                          const int32_t* counts, int32_t nclients, int32_t batch, int32_t C,
                          int32_t H, int32_t W, int32_t gh, int32_t gw, int32_t xh, int32_t xw,
                          void* stream);
/* Its weight gradient: fh_maxpool2_bwd(dpool, idx, xin = ReLU output) + fh_conv2d_wgrad in
 * one pass (the ReLU mask at the argmax is y > 0); dpool / y in planes gh x gw.  Workspace:
 * fh_conv2d_wgrad_workspace(nclients, batch, 1, h, w, cout, 3, 3, 1, 1). */
int fh_conv2d_c1_pool_wgrad(const float* x, int64_t x_cs, const float* dpool, int64_t dp_cs,
                            const uint8_t* idx, int64_t i_cs, const float* y, int64_t y_cs,
                            float* dw, int64_t dw_cs, float* db, int64_t db_cs, void* workspace,
                            size_t ws_bytes, const int32_t* counts, int32_t nclients,
                            int32_t batch, int32_t h, int32_t w_, int32_t cout, int32_t gh,
                            int32_t gw, void* stream);
/* fh_conv2d_c1_pool_wgrad without the final reduction (as fh_conv2d_wgrad_deferred): the
 * *splits_out >= 1 per-chunk partials stay in `slab` for fh_sgd_step_slabs /
 * fh_adam_step_slabs. */
int fh_conv2d_c1_pool_wgrad_deferred(const float* x, int64_t x_cs, const float* dpool,
                                     int64_t dp_cs, const uint8_t* idx, int64_t i_cs,
                                     const float* y, int64_t y_cs, float* dw, int64_t dw_cs,
                                     float* db, int64_t db_cs, void* slab, size_t slab_bytes,
                                     const int32_t* counts, int32_t nclients, int32_t batch,
                                     int32_t h, int32_t w_, int32_t cout, int32_t gh, int32_t gw,
                                     int32_t* splits_out, int64_t* bias_off_out, void* stream);
/* fh_bn_fwd_train (its apply pass: y = [relu](bn(x) [+ res]), save_mean / save_invstd,
 * running statistics) from the tiles fh_conv2d_fwd_bnstats left — FederatedResNet's stem
 * bn1 and block bn2 + residual + ReLU (models_pytorch.py:189-194, :241-242), whose output the
 * next block reads twice and is therefore materialised. */
int fh_bn_apply_tiles(const double* part, const float* x, int64_t x_cs, float* y, int64_t y_cs,
                      const float* res, int64_t res_cs, const float* gamma, const float* beta,
                      int64_t p_cs, float* running_mean, float* running_var, int64_t r_cs,
                      float* save_mean, float* save_invstd, const int32_t* counts,
                      int32_t nclients, int32_t batch, int32_t C, int32_t HW, float eps,
                      float momentum, int32_t relu, void* stream);

/* ---------------- launch planning ---------------------------------------------
 * Share of the chip (0, 1] that the split-K planners of the conv / linear entry points
 * aim to fill, for launches issued by the CALLING THREAD (thread-local; default 1).
 * A client lane running concurrently with others asks for less (fedhip/lanes.py). */
int fh_set_fill_fraction(float fraction);
float fh_get_fill_fraction(void);

/* Dual-role layer backward (CIFAR10CNN / ResNet 3x3 layers, the WGRAD + DGRAD pair of
 * models_pytorch.py's autograd backward).  mode 1 or 2 arms the CALLING THREAD's next
 * fh_conv2d_wgrad* call: a direct quadrant-wave WGRAD whose dW needs no reduction launch is
 * held and issued in one grid with the next direct DGRAD on the same stream (1: WGRAD
 * workgroups first, 2: DGRAD first), else on its own before it.  mode 0 issues anything still
 * held and disarms; call it after the pair's DGRAD.  mode -1 disarms and drops a held launch
 * unissued (a caller's error path). */
int fh_conv_pair(int32_t mode);
/* The calling thread's pairing state, for instrumentation (bench.py's per-launch timing
 * attributes a dual launch to both roles' work): *held = 1 while a WGRAD launch is held for
 * the next DGRAD, *dual_launches = dual-role grids this thread has issued so far. */
int fh_conv_pair_status(int32_t* held, int64_t* dual_launches);
/* r05: fh_conv_defer_dgrad(1) arms the calling thread's next split direct DGRAD on 16x16
 * planes with a plain sum epilogue to leave its partials unreduced; the conv1 weight gradient
 * that reads its output (fh_conv2d_c1_pool_wgrad[_deferred], fh_conv2d_c1_pool_wgrad_persample
 * [_clip]) sums them while staging (the epilogue's order: the same bits).  Any other consumer
 * path, or fh_conv_defer_dgrad(0), launches the skipped reduction first. */
int fh_conv_defer_dgrad(int32_t on);
/* r06 (instrumentation): DGRADs the calling thread left unreduced under fh_conv_defer_dgrad, and
 * how many of those partial slabs a conv1 weight-gradient consumer summed while staging. */
int fh_conv_defer_status(int64_t* deferred, int64_t* taken);
/* The next WGRAD + DGRAD pair's output gradient is a 2x2 max-pool's backward (SimpleCNN conv2,
 * models_pytorch.py:88-90, pool2 after relu(conv2)): dY(y, x) = dpool[y/2][x/2] where (y, x) is
 * the window's argmax pidx and the pooled ReLU output ypool there is > 0, else 0
 * (fh_maxpool2_bwd_ymask), pooled planes ph x ph, dense.  Call after fh_conv_pair(mode).  When
 * the pair becomes one dual-role launch on 16x16 planes both roles route dY on load and the
 * pair's dY tensor is never written; otherwise the library first fills it with
 * fh_maxpool2_bwd_ymask.  fh_conv_pair(0 / -1) disarms. */
int fh_conv_pooled_dy(const float* dpool, int64_t dp_cs, const uint8_t* pidx, int64_t pi_cs,
                      const float* ypool, int64_t yp_cs, int32_t ph);

/* Lane streams (fedhip/lanes.py; replaces the reference's one-thread-per-client
 * concurrency, federated_simulation.py:309-318).  cu_mask (nullable; mask_words 32-bit
 * words, bit i = CU i) restricts the stream to those CUs (hipExtStreamCreateWithCUMask);
 * otherwise the stream gets dispatch priority `priority` (lower = higher, HIP's range).
 * *stream_out is a hipStream_t; release it with fh_stream_destroy. */
int fh_stream_create(int32_t priority, const uint32_t* cu_mask, int32_t mask_words,
                     void** stream_out);
int fh_stream_destroy(void* stream);

/* Step programs (csrc/program.hip; replaces torch.cuda.CUDAGraph.replay for concurrent
 * lanes: +1.3 % on KT).  fh_record_begin makes this thread's libfedhip launches ALSO append
 * to a new program (kernel, geometry, LDS bytes and a private copy of the arguments);
 * fh_record_end stops it.  fh_program_launch re-issues the list on `stream`.  A program
 * owns everything it launches with except the device buffers its arguments point at.
 * fh_graph_node_counts: kernel / non-kernel work nodes of a captured hipGraph_t, so the
 * caller can verify a recording made during that capture saw the whole step. */
int fh_record_begin(void** program_out);
int fh_record_end(void* program, int32_t* kernels_out);
int fh_graph_node_counts(void* graph, int32_t* kernels_out, int32_t* others_out);

/*
 * fh_program_matches_graph: *match_out = 1 when `program` (fh_record_begin/end) is a faithful
 * copy of the captured hipGraph_t `graph`: no non-kernel work node in the graph, and the
 * graph's kernel functions equal the recorded ones as multisets.  0 otherwise (the caller
 * replays the graph).  Stronger than comparing fh_graph_node_counts with the recorded count.
 */
int fh_program_matches_graph(void* program, void* graph, int32_t* match_out);
int fh_program_launch(void* program, void* stream);
/* r06: relocation of the per-step input slot.  fh_program_relocate marks every 8-byte
 * argument word of the recorded launches (struct fields included) equal to one of ptrs[0..n),
 * each inside [base, base + len) — the step's per-step input slot and its views; *found = the
 * number of words, or -1 when some other word points into the slot (then only
 * fh_program_launch is valid).  fh_program_launch_at rewrites those words to the same offsets
 * from new_base (another row laid out like the slot) and issues the program: the step reads
 * its inputs in place, without a copy into the slot first. */
int fh_program_relocate(void* program, const uint64_t* ptrs, int32_t nptrs, uint64_t base,
                        int64_t len, int32_t* found);
int fh_program_launch_at(void* program, void* stream, uint64_t new_base);
int fh_program_destroy(void* program);

/* Launch timestamps of the dual-role conv backward (bench.py's roofline over the TIMED
 * rounds; replaces the reference's wall-clock timers around train_local_model,
 * training.py:86,140).  While rec is non-null, every dconv_wgrad_dual_kernel launch of the
 * layer shape (map w x w, cin -> cout) appends one record per workgroup to rec [cap][4]
 * uint32: its dispatch packet key, the shape key, and the workgroup's first / last wall-clock
 * tick (100 MHz counter, low 32 bits; fh_wall_clock_khz); *count (uint32, caller-zeroed) is
 * the next free record.  A launch's duration is max(last) - min(first) over its records —
 * the kernel trace's begin-to-end.  rec = null turns it off.  Host calls, outside a capture. */
int fh_launch_ts_set(void* rec, void* count, uint32_t cap, int32_t w, int32_t cin, int32_t cout);
int fh_wall_clock_khz(int32_t* khz);
/* dst[0:nbytes) = src[0:nbytes) by a kernel (16-B aligned, nbytes % 16 == 0): the per-step
 * input row copy of a lane in program mode. */
int fh_copy_bytes(const void* src, void* dst, int64_t nbytes, void* stream);

/* ---------------- on-device input pipeline (data_loader.py:298-301, 454-458) -----
 * x[z][b] = Normalize(RandomHorizontalFlip(RandomCrop(data[idx[z][b]], pad)))
 * from raw uint8 HWC images (torchvision layout) to fp32 NCHW: (u/255 - mean_c) /
 * std_c (mean/stdv: HOST float[C], C <= 4); pad 0 = no crop, flip 0 = no flip.
 * Crop/flip per image from aug_in (uchar4 {i, j, flip, -} per [z][b], stride
 * aug_cs; replay) or Philox(seed + *seed_dev, (z, b)), then recorded to aug_out
 * (nullable).  y[z][b] = labels[idx[z][b]] (y nullable). */
int fh_gather_u8(const uint8_t* data, const int64_t* labels, const int64_t* idx, int64_t idx_cs,
                 float* x, int64_t x_cs, int64_t* y, int64_t y_cs, const int32_t* counts,
                 int32_t nclients, int32_t batch, int32_t C, int32_t H, int32_t W,
                 const float* mean, const float* stdv, int32_t pad, int32_t flip,
                 const uint8_t* aug_in, uint8_t* aug_out, int64_t aug_cs, uint64_t seed,
                 const uint64_t* seed_dev, void* stream);

/* ---------------- update compression (compression.py:123-368) -----
 * Per client row z and parameter segment s = [seg_offsets[s], seg_offsets[s+1]):
 * v = x[z] - base[z] (base nullable: v = x[z]; base_cs 0 broadcasts one row) and
 * out[z] = base[z] + decompress(compress(v)) (out nullable; may alias x).
 * Segments are processed in chunks of fh_compress_chunk_elems() elements;
 * chunk_offsets[s] (device int32[nseg+1]) = cumulative ceil(len_s / chunk), nchunks =
 * chunk_offsets[nseg].
 *
 * fh_quantize_rows   QuantizationCompressor._quantize_tensor + _dequantize_tensor
 *                    (:203-244), bits in [1,16]; codes (nullable, bits <= 8) get the
 *                    uint8 wire codes; scale_out / zp_out (nullable, [C][nseg]) the
 *                    per-segment scale (double) and zero point.  Asymmetric mode on a
 *                    constant segment raises in the reference (round(inf)); here that
 *                    segment passes through unchanged and zp_out = INT64_MIN.
 *                    bits = 16: as in the reference, codes >= 32768 wrap through int16
 *                    before they are dequantised.
 * fh_topk_rows       TopKSparsificationCompressor._sparsify_tensor + _desparsify_tensor
 *                    (:327-365) with k = seg_k[s] (device int64[nseg]); keep (nullable)
 *                    gets the uint8 keep-mask.  Ties at the k-th magnitude: lowest
 *                    flat indices are kept. */
int64_t fh_compress_chunk_elems(void);
int64_t fh_quantize_workspace(int32_t nclients, int32_t nchunks);
int fh_quantize_rows(const float* x, int64_t x_cs, const float* base, int64_t base_cs, float* out,
                     int64_t out_cs, uint8_t* codes, int64_t codes_cs, int32_t nclients,
                     const int64_t* seg_offsets, const int32_t* chunk_offsets, int32_t nseg,
                     int32_t nchunks, int32_t bits, int32_t symmetric, double* scale_out,
                     int64_t* zp_out, void* ws, size_t ws_bytes, void* stream);
int64_t fh_topk_workspace(int32_t nclients, int32_t nseg, int32_t nchunks);
int fh_topk_rows(const float* x, int64_t x_cs, const float* base, int64_t base_cs, float* out,
                 int64_t out_cs, uint8_t* keep, int64_t keep_cs, int32_t nclients,
                 const int64_t* seg_offsets, const int32_t* chunk_offsets, const int64_t* seg_k,
                 int32_t nseg, int32_t nchunks, void* ws, size_t ws_bytes, void* stream);

/* ---------------- error feedback and stochastic rounding (not in the reference) -----
 * Same conventions as the block above: packed rows with element strides, base nullable
 * (base_cs 0 broadcasts one row), segments by seg_offsets / chunk_offsets, nothing outside
 * [seg_offsets[0], seg_offsets[nseg]) of a row is read or written, one launch per stage for all
 * clients.  fl32() marks one rounded fp32 operation; none is ever fused with another.
 *
 * Error feedback (Stich et al. 2018; Karimireddy et al. 2019): resid[z] is client z's residual
 * row, what compression has removed from its earlier updates.
 *
 * fh_ef_fold          resid[z][i] = fl32( fl32(x[z][i] - base[z][i]) + resid[z][i] )
 *                     (base NULL: fl32(x + resid)).  The result is called v below.
 * fh_ef_topk_finish   after fh_topk_rows(x = resid, base = NULL, out = NULL, keep) has written
 *                     the uint8 keep mask of v:  d = keep ? v : +0.0,
 *                     x_out = fl32(base + d) (base NULL: d),  resid = keep ? +0.0 : v.
 *                     That is fh_topk_rows' own output for an update whose delta is v: a kept
 *                     coordinate carries fl32(base + v), a dropped one base (a base of -0.0
 *                     comes out +0.0, as there).  The tie rule is fh_topk_rows'.
 * fh_ef_quant_finish  after fh_quantize_rows(x = resid, base = NULL, out = c) has written the
 *                     dequantised v:  x_out = fl32(base + c) (base NULL: c),
 *                     resid = fl32(v - c).  x_out may be c.
 *
 * fh_squant_rows      stochastic-rounding quantiser (QSGD, Alistarh et al. 2017), bits in
 *                     [2, 16], per (client row, segment).  v = x - base (base NULL: x), or, when
 *                     resid is given, v = resid (fh_ef_fold ran first; x is not read).
 *   symmetric:   a = max|v|, qmax = 2^(bits-1) - 1, scale = fl32(a / qmax), t = fl32(v / scale),
 *                q = clamp(floor(t) + up, -qmax, qmax), deq = fl32(q * scale)
 *   asymmetric:  lo = min v, hi = max v, L = 2^bits - 1, scale = fl32(fl32(hi - lo) / L),
 *                t = fl32(fl32(v - lo) / scale), q = clamp(floor(t) + up, 0, L),
 *                deq = fl32(lo + fl32(q * scale))
 *   up:          f = fl32(t - floor(t)) (exact except for a tiny negative t, where it rounds
 *                to 1), thr = (uint32)(f * 2^24), up = (r >> 8) < thr — an integer compare, no
 *                transcendental.  Divisions are IEEE round-to-nearest.
 *   r:           the element's 32-bit random word.  For flat row index i it is word i & 3 of
 *                Philox4x32-10(key, ctr_hi = ids[z] | FH_SQUANT_STREAM_BIT, ctr_lo = i >> 2),
 *                ids: device int64[nclients], the global client ids (below 2^62).  The bit
 *                keeps the stream apart from the update-level DP noise (ctr_hi = id under the
 *                same round key) and from the FH_DPFA_STREAM_* words (bit 63 set).  words
 *                (nullable, uint32 rows with stride words_cs, indexed like x) replaces the
 *                draw: r = words[z][i] (exact replay).
 *   scale == 0:  (all-zero segment, constant segment in asymmetric mode, one element) the
 *                segment passes through: deq = v, codes 0.
 *   outputs:     out = fl32(base + deq) (base NULL: deq; nullable; may alias x);
 *                codes (nullable, bits <= 8): uint8 q + qmax (symmetric) or q (asymmetric);
 *                scale_out / lo_out (nullable, fp32 [nclients][nseg]; lo_out = 0 in symmetric
 *                mode); resid_out (nullable; may alias resid) = fl32(v - deq).
 *   Non-finite inputs: unspecified.  ws: fh_squant_workspace(nclients, nchunks) bytes. */
#define FH_SQUANT_STREAM_BIT (1ull << 62)
int fh_ef_fold(const float* x, int64_t x_cs, const float* base, int64_t base_cs, float* resid,
               int64_t resid_cs, int32_t nclients, const int64_t* seg_offsets,
               const int32_t* chunk_offsets, int32_t nseg, int32_t nchunks, void* stream);
int fh_ef_topk_finish(const float* base, int64_t base_cs, const uint8_t* keep, int64_t keep_cs,
                      float* resid, int64_t resid_cs, float* x_out, int64_t x_out_cs,
                      int32_t nclients, const int64_t* seg_offsets, const int32_t* chunk_offsets,
                      int32_t nseg, int32_t nchunks, void* stream);
int fh_ef_quant_finish(const float* base, int64_t base_cs, const float* c, int64_t c_cs,
                       float* resid, int64_t resid_cs, float* x_out, int64_t x_out_cs,
                       int32_t nclients, const int64_t* seg_offsets, const int32_t* chunk_offsets,
                       int32_t nseg, int32_t nchunks, void* stream);
int64_t fh_squant_workspace(int32_t nclients, int32_t nchunks);
int fh_squant_rows(const float* x, int64_t x_cs, const float* base, int64_t base_cs,
                   const float* resid, int64_t resid_cs, float* out, int64_t out_cs,
                   uint8_t* codes, int64_t codes_cs, float* resid_out, int64_t resid_out_cs,
                   int32_t nclients, const int64_t* seg_offsets, const int32_t* chunk_offsets,
                   int32_t nseg, int32_t nchunks, int32_t bits, int32_t symmetric, uint64_t key,
                   const int64_t* ids, const uint32_t* words, int64_t words_cs, float* scale_out,
                   float* lo_out, void* ws, size_t ws_bytes, void* stream);

/* ---------------- sparse top-k updates (compression.py:262-365) -----
 * What TopKSparsificationCompressor ships per layer, {'values', 'indices'}, as packed rows, and
 * the aggregation from it.  Conventions of the two blocks above: packed rows with element
 * strides, segments by seg_offsets / chunk_offsets, nothing outside
 * [seg_offsets[0], seg_offsets[nseg]) of a parameter row is read or written, one launch (pack:
 * two) for all clients.  fl32() marks one rounded fp32 operation; none is ever fused.
 *
 * Payload.  koff (device int32[nseg+1]) is the exclusive prefix sum of seg_k and K = koff[nseg].
 * Client z's payload is idx[z][0..K) (int32, segment-local flat index) and val[z][0..K) (fp32);
 * segment s occupies [koff[s], koff[s+1]) with indices STRICTLY ASCENDING.  Nothing outside
 * [0, K) of a payload row is read or written.
 *
 * fh_topk_pack_rows      ordered compaction of the uint8 keep mask fh_topk_rows wrote.  For every
 *                        element i of segment s with keep[z][i] != 0, in ascending i:
 *                          idx = i - seg_offsets[s],  val = v,
 *                          v = fl32(x[z][i] - base[z][i])   (base NULL: v = x[z][i]; base_cs 0
 *                        broadcasts one row) — the v fh_topk_rows ranked.  count_out (nullable,
 *                        int32 [nclients][nseg]) gets the number of kept elements found
 *                        (= seg_k[s] for finite input).  Slots of a segment beyond its count are
 *                        left untouched; kept elements beyond koff[s+1] - koff[s] are counted and
 *                        not written.  Positions come from per-(chunk, client) counts, their sum
 *                        over the segment's earlier chunks and a wave ballot / prefix popcount:
 *                        no atomics, the output is deterministic.
 *                        ws: fh_topk_pack_workspace(nclients, nchunks) bytes.
 * fh_sparse_validate     bad_out[z][s] (int32 [nclients][nseg]) = 1 when segment s of client z
 *                        holds an index < 0, an index >= seg_lens[s] (device int64[nseg]) or a
 *                        neighbouring pair that is not strictly ascending, else 0.  Integer
 *                        compares on idx alone.  The two consumers below take VALIDATED payloads
 *                        only; on any other payload their result is unspecified (they still
 *                        write nothing outside the rows' covered range).
 * fh_sparse_unpack_rows  _desparsify_tensor plus the base:
 *                          d[z][i] = val[z][p] where idx[z][p] names i, +0.0 elsewhere,
 *                          out[z][i] = fl32(base[z][i] + d[z][i])   (base NULL: d[z][i]).
 *                        That is fh_topk_rows' own out (a base of -0.0 comes out +0.0 where
 *                        nothing is kept).  out may alias base only when base_cs != 0.
 * fh_sparse_fedavg       base is ONE row (the global model), out one row, neither aliasing the
 *                        other.  For every j of the covered range
 *                          acc = accumulate ? out[j] : +0.0
 *                          for k = 0 .. num_clients-1, r = row_index[k] (NULL: k):
 *                            xk  = fl32(base[j] + d[r][j])
 *                            acc = fl32(acc + fl32(weights[k] * xk))
 *                          out[j] = acc
 *                        — bit for bit fh_fedavg_weighted_sum over the rows
 *                        fh_sparse_unpack_rows(base broadcast) would write, without them.
 *                        Bytes moved: 8 per payload entry, 8 per parameter. */
int64_t fh_topk_pack_workspace(int32_t nclients, int32_t nchunks);
int fh_topk_pack_rows(const float* x, int64_t x_cs, const float* base, int64_t base_cs,
                      const uint8_t* keep, int64_t keep_cs, int32_t* idx, int64_t idx_cs,
                      float* val, int64_t val_cs, int32_t* count_out, int32_t nclients,
                      const int64_t* seg_offsets, const int32_t* chunk_offsets,
                      const int32_t* koff, int32_t nseg, int32_t nchunks, void* ws,
                      size_t ws_bytes, void* stream);
int fh_sparse_validate(const int32_t* idx, int64_t idx_cs, int32_t nclients,
                       const int64_t* seg_lens, const int32_t* koff, int32_t nseg,
                       int32_t* bad_out, void* stream);
int fh_sparse_unpack_rows(const int32_t* idx, int64_t idx_cs, const float* val, int64_t val_cs,
                          const float* base, int64_t base_cs, float* out, int64_t out_cs,
                          int32_t nclients, const int64_t* seg_offsets,
                          const int32_t* chunk_offsets, const int32_t* koff, int32_t nseg,
                          int32_t nchunks, void* stream);
int fh_sparse_fedavg(const int32_t* idx, int64_t idx_cs, const float* val, int64_t val_cs,
                     const int32_t* row_index, const float* weights, int32_t num_clients,
                     const float* base, const int64_t* seg_offsets, const int32_t* chunk_offsets,
                     const int32_t* koff, int32_t nseg, int32_t nchunks, float* out,
                     int32_t accumulate, void* stream);

/* ---------------- packed quantised updates (compression.py:138-244) -----
 * What QuantizationCompressor ships per layer, a uint8 code per element plus {scale, zero_point},
 * as bit-packed code rows, and the aggregation from it.  The deterministic quantiser
 * (fh_quantize_rows) with bits in [1, 8] only.  Conventions of the blocks above: device pointers
 * with element strides, base nullable (base_cs 0 broadcasts one row), segments by seg_offsets /
 * chunk_offsets, nothing outside [seg_offsets[0], seg_offsets[nseg]) of a parameter row is read or
 * written, one launch for all clients, no atomics, no host sync.  fl32() marks one rounded fp32
 * operation; none is ever fused.
 *
 * Payload.  A code occupies cw bits: cw = 1 for bits 1, 2 for bits 2, 4 for bits 3..4, 8 for bits
 * 5..8.  Element j (segment-local) of segment s sits in byte boff[s] + (j * cw) / 8 of a client's
 * code row, at bits [(j * cw) % 8, (j * cw) % 8 + cw), low bits first.  boff (device
 * int64[nseg+1]) is the exclusive prefix sum of ceil(len_s * cw / 8) rounded up to 16; B =
 * boff[nseg].  Code rows must be 16-byte aligned with a row stride (bytes) that is a multiple of
 * 16, else FH_E_INVALID: every load of codes is an aligned vector load.  Nothing outside a
 * segment's ceil(len_s * cw / 8) bytes of a code row is read or written (the padding up to the
 * next 16-byte boundary included).  fp32 parameter rows keep their usual freedom: any 4-byte
 * alignment, any stride, segments starting anywhere.
 * Next to the codes, [nclients][nseg] each and contiguous: scale (double) and zp (int64) exactly
 * as fh_quantize_rows writes scale_out / zp_out, and passv (fp32).
 *
 * Dequantisation (quant_apply_kernel's arithmetic):
 *     d = fl32( fl32( (float)code - (float)zp ) * (float)scale )
 * An all-zero symmetric segment has code 0 and d = -0.0 ((0 - 127) * 0): no special case.
 * Pass-through.  zp == INT64_MIN marks a segment fh_quantize_rows passed through (asymmetric mode
 * on a constant segment).  With finite input its v are numerically equal and differ at most in
 * the sign of zero: the payload carries passv = v of the segment's first element and code = sign
 * bit of v per element, and d = the magnitude bits of passv under bit 0 of the code as sign.
 * Non-finite input: unspecified, as for fh_quantize_rows.
 *
 * fh_quant_pack_rows    codes: the uint8 rows fh_quantize_rows wrote (one code per element,
 *                       indexed like x, stride codes_cs); zp: its zp_out; x / base: the same as
 *                       in that call.  Writes packed (the code rows) and passv.  One thread
 *                       assembles whole bytes; the unused high bits of a segment's last byte are
 *                       written as zero, the padding bytes are not written.  A flagged segment
 *                       reads v = fl32(x[z][i] - base[z][i]) (base NULL: x[z][i]) instead of the
 *                       codes; passv of an unflagged segment is written as +0.0.
 * fh_quant_validate     bad_out[z][s] (int32 [nclients][nseg]) = 1 when segment s of client z
 *                       holds a code >= 2^bits (possible only where bits < cw), when scale is not
 *                       finite or is negative, or when the segment is flagged and passv is not
 *                       finite; else 0.  seg_lens: device int64[nseg].  Padding bits and bytes
 *                       are not looked at.  The two consumers below take VALIDATED payloads only;
 *                       on any other payload their result is unspecified (they still write
 *                       nothing outside the rows' covered range).
 * fh_quant_unpack_rows  out[z][i] = fl32(base[z][i] + d[z][i])   (base NULL: d[z][i]) — that is
 *                       fh_quantize_rows' own out.  out may alias base only when base_cs != 0.
 * fh_quant_fedavg       base is ONE row (the global model) or NULL, out one row, neither aliasing
 *                       the other.  For every j of the covered range
 *                         acc = accumulate ? out[j] : +0.0
 *                         for k = 0 .. num_clients-1, r = row_index[k] (NULL: k):
 *                           xk  = fl32(base[j] + d[r][j])        (base NULL: d[r][j])
 *                           acc = fl32(acc + fl32(weights[k] * xk))
 *                         out[j] = acc
 *                       — bit for bit fh_fedavg_weighted_sum over the rows fh_quant_unpack_rows
 *                       (base broadcast) would write, without them.
 *                       Bytes moved: cw / 8 per element and client, 8 per parameter. */
int fh_quant_pack_rows(const uint8_t* codes, int64_t codes_cs, const int64_t* zp, const float* x,
                       int64_t x_cs, const float* base, int64_t base_cs, uint8_t* packed,
                       int64_t packed_cs, float* passv, int32_t nclients,
                       const int64_t* seg_offsets, const int32_t* chunk_offsets,
                       const int64_t* boff, int32_t nseg, int32_t nchunks, int32_t bits,
                       void* stream);
int fh_quant_validate(const uint8_t* packed, int64_t packed_cs, const double* scale,
                      const int64_t* zp, const float* passv, int32_t nclients,
                      const int64_t* seg_lens, const int64_t* boff, int32_t nseg, int32_t bits,
                      int32_t* bad_out, void* stream);
int fh_quant_unpack_rows(const uint8_t* packed, int64_t packed_cs, const double* scale,
                         const int64_t* zp, const float* passv, const float* base,
                         int64_t base_cs, float* out, int64_t out_cs, int32_t nclients,
                         const int64_t* seg_offsets, const int32_t* chunk_offsets,
                         const int64_t* boff, int32_t nseg, int32_t nchunks, int32_t bits,
                         void* stream);
int fh_quant_fedavg(const uint8_t* packed, int64_t packed_cs, const double* scale,
                    const int64_t* zp, const float* passv, const int32_t* row_index,
                    const float* weights, int32_t num_clients, const float* base,
                    const int64_t* seg_offsets, const int32_t* chunk_offsets, const int64_t* boff,
                    int32_t nseg, int32_t nchunks, int32_t bits, float* out, int32_t accumulate,
                    void* stream);

/* ---------------- evaluation metrics (training.py:214-242, 307-360) ----------
 * Eval-mode metrics of [nclients][batch][K] logits: per image the first-index
 * argmax (torch.max) and the CE loss.  loss_sum[z] += sum of the slot's image
 * losses (fp64) and correct[z] += its correct predictions (both nullable,
 * accumulated across calls); class_correct[k] / class_total[k] (nullable
 * together) count correct and seen images of label k (integer atomics). */
int fh_eval_metrics(const float* logits, int64_t l_cs, const int64_t* targets, int64_t t_cs,
                    const int32_t* counts, int32_t nclients, int32_t batch, int32_t num_classes,
                    double* loss_sum, int64_t* correct, int64_t* class_correct,
                    int64_t* class_total, void* stream);

/* ---------------- AdaptiveAvgPool2d((1,1)) --------------------------------- */
int fh_avgpool_fwd(const float* x, int64_t x_cs, float* y, int64_t y_cs, const int32_t* counts,
                   int32_t nclients, int32_t batch, int32_t C, int32_t HW, void* stream);
int fh_avgpool_bwd(const float* dy, int64_t dy_cs, float* dx, int64_t dx_cs,
                   const int32_t* counts, int32_t nclients, int32_t batch, int32_t C, int32_t HW,
                   void* stream);

/* ---------------- depthwise 3x3 convolution (groups = channels) ------------
 * LightweightMobileNet's depthwise layers (models_pytorch.py DepthwiseSeparableConv): no bias,
 * x: [clients][batch][C][h][w]; w: [C][1][3][3] per client (any 4-byte aligned offset of a
 * packed parameter row); y: [clients][batch][C][h/stride][w/stride].  Supported: 3x3, pad 1,
 * stride 1 or 2, square maps of 8, 16 or 32, C % 8 == 0, activations 16-byte aligned with
 * client strides % 4 == 0; anything else returns FH_E_UNSUPPORTED.  Images >= counts[client]
 * are neither read nor written.  Deterministic (no atomics); plain fp32 multiply-adds. */
int fh_dwconv3x3_fwd(const float* x, int64_t x_cs, const float* w, int64_t w_cs, float* y,
                     int64_t y_cs, const int32_t* counts, int32_t nclients, int32_t batch,
                     int32_t C, int32_t h, int32_t w_, int32_t kh, int32_t kw, int32_t stride,
                     int32_t pad, void* stream);
/* h / w_: the INPUT map (dx); dy is [C][h/stride][w_/stride].  accumulate = 1: dx += result. */
int fh_dwconv3x3_dgrad(const float* dy, int64_t dy_cs, const float* w, int64_t w_cs, float* dx,
                       int64_t dx_cs, const int32_t* counts, int32_t nclients, int32_t batch,
                       int32_t C, int32_t h, int32_t w_, int32_t kh, int32_t kw, int32_t stride,
                       int32_t pad, int32_t accumulate, void* stream);
/* dw is overwritten.  With few (client, channel) pairs the sum is split over image ranges
 * through `workspace` (>= fh_dwconv3x3_wgrad_workspace(...) bytes; 0 = never splits; a NULL /
 * too-small workspace disables the split) and the partials are added in split order by a
 * second launch. */
size_t fh_dwconv3x3_wgrad_workspace(int32_t nclients, int32_t batch, int32_t C, int32_t h,
                                    int32_t w_, int32_t stride);
int fh_dwconv3x3_wgrad(const float* x, int64_t x_cs, const float* dy, int64_t dy_cs, float* dw,
                       int64_t dw_cs, void* workspace, size_t ws_bytes, const int32_t* counts,
                       int32_t nclients, int32_t batch, int32_t C, int32_t h, int32_t w_,
                       int32_t kh, int32_t kw, int32_t stride, int32_t pad, void* stream);

/* ---------------- on-device batch assembly (DataLoader replacement) -------
 * x[z][b] = data[idx[z*idx_cs+b]], y[z][b] = labels[idx[..]] for b < counts[z]. */
int fh_gather_batch(const float* data, const int64_t* labels, const int64_t* idx, int64_t idx_cs,
                    float* x, int64_t x_cs, int64_t* y, int64_t y_cs, int64_t sample_elems,
                    const int32_t* counts, int32_t nclients, int32_t batch, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FEDHIP_H_ */
