/*
 * ldpc_sparc_amd.h -- C ABI of libldpc_sparc_amd.so, the MI355X (gfx950)
 * AMP/BP decoding engine behind the reference's Python call surface.
 *
 * Conventions
 *   - every entry point returns 0 on success and a negative code on failure
 *     (no C++ exceptions cross the ABI); sg_last_error() describes the last
 *     failure on the calling thread;
 *   - "host" entry points take caller-owned host buffers and block until the
 *     result is back in them; "_device" entry points take device pointers and
 *     a hipStream_t (NULL = the library's stream for the current device) and
 *     return without synchronising;
 *   - handles (sg_graph, sg_amp_plan, sg_comm) own device memory and belong to
 *     the device that was current when they were created; one process per GPU.
 *   - the library has no CPU decode path: without a visible gfx950 device every
 *     decode entry point fails with SG_ERR_NO_DEVICE.
 *
 * Reference interfaces replaced are cited per entry point (path:line under the
 * reference repository SophieLangdon27/LDPC_SPARC).
 */
#ifndef LDPC_SPARC_AMD_H
#define LDPC_SPARC_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum sg_status {
    SG_OK = 0,
    SG_ERR_INVALID = -2,   /* bad argument (shape, degree, enum) */
    SG_ERR_BAD_ARG = SG_ERR_INVALID, /* the same code under its other name */
    SG_ERR_NO_DEVICE = -3, /* no usable GPU */
    SG_ERR_HIP = -4,       /* HIP runtime failure */
    SG_ERR_NOMEM = -5,     /* allocation failure (the reference returns -1 here, c_ldpc.c:41) */
    SG_ERR_UNSUPPORTED = -6,
    SG_ERR_COMM = -7       /* RCCL failure */
};

enum sg_dectype { SG_SUMPROD = 0, SG_SUMPROD2 = 1, SG_MINSUM = 2 };
enum sg_precision { SG_F64 = 0, SG_F32 = 1 };

/* ---------------------------------------------------------------- runtime */
const char *sg_last_error(void);
const char *sg_version(void);
int sg_device_count(int *count);
int sg_device_cu_count(int *cus); /* compute units of the current device */
int sg_set_device(int device);
int sg_get_stream(void **stream);           /* library stream of the current device */
int sg_malloc(void **dptr, size_t bytes);
int sg_free(void *dptr);
int sg_memcpy_h2d(void *dst, const void *src, size_t bytes, void *stream);
int sg_memcpy_d2h(void *dst, const void *src, size_t bytes, void *stream);
int sg_memset(void *dptr, int value, size_t bytes, void *stream);
int sg_stream_synchronize(void *stream);
/* An extra non-blocking stream (concurrent batches on one GPU). */
int sg_stream_create(void **stream);
int sg_stream_destroy(void *stream);

/* HIP events on a given stream (bench.py times the kernels on the stream they
 * run on, not on torch's current stream). */
int sg_event_create(void **ev);
int sg_event_destroy(void *ev);
int sg_event_record(void *ev, void *stream);
int sg_event_elapsed_ms(void *start, void *stop, float *ms);
int sg_device_synchronize(void);

/* Per-phase kernel timing.  When enabled, every kernel launch of the decoders
 * is bracketed by HIP events on the stream it is launched on; collect
 * synchronises the pending events, returns the summed milliseconds and the
 * launch count per phase (arrays of SG_PH_COUNT) and resets the counters.
 * on = 2 records only the per-iteration scope of the split per-codeword
 * engine, not its per-kernel scopes inside it: every timed event record on a
 * stream holds the next kernel back by several microseconds, so bench.py's
 * timed region brackets each iteration (two events) rather than each of its
 * four kernels. */
enum sg_phase {
    SG_PH_AB_A = 0, SG_PH_AB_B = 1, SG_PH_AZ_A = 2, SG_PH_AZ_B = 3, SG_PH_ETA = 4,
    SG_PH_CONTROL = 5, SG_PH_BP = 6, SG_PH_DENSE = 7, SG_PH_AMP_CW = 8, SG_PH_CW2_AB = 9, SG_PH_CW2_AZ = 10,
    SG_PH_CW2_CTRL = 11,
    /* integrated decoders on the DCT design: BP output -> beta (probabilities, bp_to_beta, update, ||beta||^2)
     * and the differentiated eta */
    SG_PH_INT_GLUE = 12, SG_PH_INT_DETA = 13, SG_PH_COUNT = 14
};
int sg_profile_enable(int on);
int sg_profile_collect(double *total_ms, int64_t *launches);
const char *sg_phase_name(int phase);

/* ------------------------------------------------------- dense design AMP */
typedef struct sg_dense_plan sg_dense_plan;

/* Dense Gaussian design A [n][L*M] row-major (create_design_matrix,
 * sparc_new.py:1284-1294: default_rng(seed).normal(0, 1/sqrt(n))), uploaded
 * once and shared by every codeword of a batch.  P is the total power
 * (nonzero entries sqrt(n P / L), sparc_new.py:45-46).  SG_F32 runs the two
 * products as matrix-core GEMMs (v_mfma_f32_32x32x2_f32); SG_F64 is the
 * parity path.  _random draws A on the device (Philox4x32-10 + Box-Muller,
 * statistically equal to the reference's draw, not bitwise) for throughput runs. */
int sg_dense_plan_create(const double *A, int n, int L, int M, double P, int precision, sg_dense_plan **out);
int sg_dense_plan_create_random(int n, int L, int M, double P, uint64_t seed, int precision,
                                sg_dense_plan **out);
int sg_dense_plan_destroy(sg_dense_plan *p);
int sg_dense_plan_info(const sg_dense_plan *p, int *n, int *L, int *M, int *nsplit);
/* Batched AMP with fixed t_max iterations (sparc_new.py:885-912, one call per
 * codeword in the reference): y [B][n] -> soft estimate beta [B][L*M] and
 * effective observation s [B][L*M] (the reference's return values). */
int sg_dense_amp(sg_dense_plan *p, const double *y, int B, int t_max, double *beta, double *s);
int sg_dense_amp_device(sg_dense_plan *p, const void *d_y, int B, int t_max, void *d_beta, void *d_s,
                        void *stream);
/* One iteration from a given state (sparc_amp_single_it, sparc_new.py:975-990):
 * y [n], beta [L*M], z [n], tau_sqr -> beta', z', tau_sqr'. */
int sg_dense_amp_iteration(sg_dense_plan *p, const double *y, const double *beta, const double *z,
                           double tau_sqr, double *beta_out, double *z_out, double *tau_sqr_out);
/* Device pointers of the plan's own beta and s [B][L*M] after the last
 * sg_dense_amp_device call (valid until the next call; lets a pipeline feed
 * the glue without copies). */
int sg_dense_state_device(sg_dense_plan *p, void **d_beta, void **d_s);
/* Device pointer of the plan's design matrix A [n][L*M] (row-major, the
 * plan's precision, no padding) -- lets a checker read A back in row blocks
 * (tests/test_c5_full_gpu.py) without a second copy. */
int sg_dense_plan_matrix_device(const sg_dense_plan *p, const void **d_A);
/* x = A beta0 for one-hot beta0 (section index d_idx [B][L], value sqrt(n P / L)). */
int sg_dense_encode_device(sg_dense_plan *p, const int32_t *d_idx, int B, void *d_x, void *stream);
/* MAP section indices of s [B][L*M] (msg_vector_map_estimator, sparc_new.py:1099-1116). */
int sg_dense_map_device(sg_dense_plan *p, const void *d_s, int B, int32_t *d_idx, void *stream);
/* AMP -> BP glue (beta_estimate_to_bp_probs, sparc_new.py:1118-1138, then the
 * clip and log of ldpc_bp :1167-1169): for sections [l0, l0+nl) of beta
 * [B][L*M], bit LLRs (MSB first, positive => 0) at d_llr[b*llr_ld + (l-l0)*log2 M + i],
 * or the bit-0 probabilities themselves when probs_only. */
int sg_beta_to_llr_device(int precision, const void *d_beta, int B, int L, int M, double sqrt_nPl, int l0,
                          int nl, int llr_ld, int probs_only, void *d_llr, void *stream);

/* Error counts of the concatenated scheme (sparc_sim_new.py:12-23):
 * unprotected bits from MAP indices d_map_idx [B][L] (first L_unprotected
 * sections) against d_true_idx, protected bits app[:K] < 0 of each of the
 * `mults` BP blocks (d_app [B*mults][N]) against d_info [B][mults*K].  Adds
 * {codewords, bit errors, codeword errors, unprotected bit errors, protected
 * bit errors} into d_counts[5]. */
int sg_concat_count_errors_device(int precision, const int32_t *d_map_idx, const int32_t *d_true_idx, int B,
                                  int L, int L_unprotected, int logM, const void *d_app, const uint8_t *d_info,
                                  int mults, int N, int K, int64_t *d_counts, void *stream);
/* BP result -> known sections of the three-stage concatenated decoder (AMP -> BP -> AMP with the BP-decoded
 * sections known, sg_amp_decode_partial_device): from the BP output d_app [B*mults][N] (`precision`) and its
 * stopping iterations d_it [B*mults] of a decode with `max_it` iterations, d_known_idx [B][L] = -1 for the
 * L_unprotected first sections; for protected section l the MSB-first index formed from the hard decisions
 * app < 0 of its logM bits (bit i of section l is bit (l - L_unprotected) logM + i of the codeword's mults*N
 * protected bits), provided every LDPC block that holds one of those bits stopped on its syndrome
 * (it < max_it) -- a section straddles two blocks when logM does not divide N -- and -1 otherwise.  Needs no
 * graph handle.  SG_ERR_INVALID when the protected sections do not fit the blocks.  For a K-PSK codeword call it
 * with logM = log2 M + log2 K: it then yields the known section words in the layout sg_psk_pack_sections_device
 * writes (sg_psk_unpack_sections_device turns them into the known_idx / known_sym of
 * sg_camp_decode_partial_device). */
int sg_concat_known_sections_device(int precision, const void *d_app, const int32_t *d_it, int max_it, int B,
                                    int mults, int N, int L, int L_unprotected, int logM, int32_t *d_known_idx,
                                    void *stream);

/* ------------------------------------------------------------- multi-GPU */
/* One RCCL communicator per process (one process per GPU).  Rank 0 creates
 * the 128-byte unique id, the launcher distributes it, every rank calls init.
 * New capability: the reference parallelises only by independent processes
 * (ldpc_jossy/py/ldpc_awgn.py:125-131). */
typedef struct sg_comm sg_comm;
int sg_comm_unique_id(void *id_out /* 128 bytes */);
int sg_comm_init(int nranks, int rank, const void *id, sg_comm **out);
int sg_comm_allreduce_sum_i64(sg_comm *c, int64_t *d_buf, size_t count, void *stream);
int sg_comm_info(sg_comm *c, int *nranks, int *device); /* ranks and device as RCCL sees them */
int sg_comm_destroy(sg_comm *c);

/* ------------------------------------------------------------------- LDPC */
typedef struct sg_graph sg_graph;

/* Upload a Tanner graph in the reference layout (ldpc.py:303-396): vdeg[nv],
 * cdeg[nc], intrlv[nmsg] mapping variable ports to check-ordered message
 * indices.  Validates that intrlv is a permutation and the degree sums match. */
int sg_ldpc_graph_create(const int64_t *vdeg, const int64_t *cdeg, const int64_t *intrlv, int nv,
                         int nc, int nmsg, sg_graph **out);
int sg_ldpc_graph_destroy(sg_graph *g);
int sg_ldpc_graph_info(const sg_graph *g, int *nv, int *nc, int *nmsg, int *max_cdeg,
                       int *max_vdeg);
/* Name of the kernel sg_ldpc_decode(_device) launches for this graph, decoder
 * type and precision, as rocprofv3 lists it (e.g. "bp_grouped_minsum_kernel<4, 2>"
 * for the degree-grouped single-precision min-sum kernel, "bp_flood_kernel<float,
 * 1, 8, 4>" for the table kernel); NUL-terminated, truncated to len bytes. */
int sg_ldpc_decode_kernel(const sg_graph *g, int dectype, int precision, char *name, size_t len);
/* The degree-grouped layout the single-precision min-sum kernel would use for
 * a graph (bp.hpp BpGrpArgs), computed on the host with no device: info[10] =
 * {grouped (1) or table kernel (0), variable / check groups per wave, the
 * kernel instance's groups per wave (2), message image bytes, port-table
 * entries, variable-group pairs, meta and vmap lengths}; meta / vmap / vtab are
 * copied out when non-null (call once with nulls for the sizes).  pairs: run
 * equal-degree variable groups in pairs (the decode default; SG_BP_PAIR=0
 * turns it off there).  For tests that emulate the kernel on the CPU. */
int sg_ldpc_grouped_layout(const int64_t *vdeg, const int64_t *cdeg, const int64_t *intrlv, int nv, int nc,
                           int nmsg, int pairs, int32_t *info, int32_t *meta, int meta_cap, int32_t *vmap,
                           int vmap_cap, uint16_t *vtab, int vtab_cap);

/* Batched flooding BP (replaces one c_ldpc.c sumprod/sumprod2/minsum call per
 * codeword, c_ldpc.c:32,138,339; driven serially by ldpc.py:463-490 and
 * sparc_new.py:1176-1179).  ch/app are row-major [B][nv] LLRs, it[B] receives
 * the reference's return value per codeword (0-based index of the stopping
 * iteration, or max_it).  minsum uses the corrected check indexing
 * (DESIGN.md "minsum") and `corr` as the normalisation factor (reference
 * default 0.7, ldpc.py:463).  precision SG_F64 reproduces the reference's
 * double arithmetic; SG_F32 is the throughput path. */
int sg_ldpc_decode(sg_graph *g, int dectype, int precision, const double *ch, int B, int max_it,
                   double corr, double *app, int32_t *it);
/* Device variant: d_ch/d_app are float or double per `precision`.  SG_F32
 * min-sum on a graph of the degree-grouped layout (bp_grouped.hip) expects
 * NaN-free channel LLRs and saturates them at +-1e30 (so +-inf decodes as
 * +-1e30); the host entry point above sends a batch holding a NaN, an
 * infinity or a value that overflows float to the table kernel instead. */
int sg_ldpc_decode_device(sg_graph *g, int dectype, int precision, const void *d_ch, int B,
                          int max_it, double corr, void *d_app, int32_t *d_it, void *stream);
/* Layered (row-serial) schedule (DESIGN.md "Layered schedule"): layer l is the
 * checks [l*layer, (l+1)*layer); an iteration takes the layers in ascending
 * order, each check computing Q_k = app[v_k] - R[c,k], the new check messages
 * R'[c,.] from Q (minsum: Lxfb without correction, times `corr`; sumprod2:
 * Lxfb with Lxor's correction) and app[v_k] = Q_k + R'[c,k] at once.  After the
 * last layer the syndrome of the hard decisions app < 0 stops the codeword:
 * it[b] is the 0-based index of that iteration, else max_it; app is as the last
 * executed layer left it.  For a quasi-cyclic code layer = z.
 *
 * sg_ldpc_layer_check (host only, no device): SG_OK when `layer` divides nc and
 * no variable occurs twice within a layer, else SG_ERR_INVALID with the first
 * offending layer and variable in sg_last_error(). */
int sg_ldpc_layer_check(const int64_t *vdeg, const int64_t *cdeg, const int64_t *intrlv, int nv, int nc,
                        int nmsg, int layer);
/* As sg_ldpc_decode / sg_ldpc_decode_device on the layered schedule.  The layer
 * size is validated as by sg_ldpc_layer_check at first use of a (graph, layer)
 * pair and its tables are kept on the graph handle.  SG_ERR_INVALID: max_it < 1,
 * a layer size that fails the check.  SG_ERR_UNSUPPORTED, before anything is
 * launched: SG_SUMPROD (the tanh form), a check degree above 32, more than
 * 65536 variables, a graph whose app, messages and tables exceed one
 * workgroup's 160 KB of LDS at this precision. */
int sg_ldpc_decode_layered(sg_graph *g, int dectype, int precision, int layer, const double *ch, int B,
                           int max_it, double corr, double *app, int32_t *it);
int sg_ldpc_decode_layered_device(sg_graph *g, int dectype, int precision, int layer, const void *d_ch, int B,
                                  int max_it, double corr, void *d_app, int32_t *d_it, void *stream);
/* Name of the kernel the layered entry points launch (e.g.
 * "bp_layered_kernel<float, 2, 8, 128>"), as sg_ldpc_decode_kernel. */
int sg_ldpc_decode_layered_kernel(const sg_graph *g, int dectype, int precision, int layer, char *name,
                                  size_t len);
/* Device-side error counting against known codewords (ldpc_awgn.py:97-104):
 * d_x[B][nv] uint8 transmitted bits, app from sg_ldpc_decode_device.  Adds to
 * d_counts[4] = {bit errors over nv, frame errors, bit errors over the first
 * k (systematic) bits, sum of it}. */
int sg_ldpc_count_errors_device(sg_graph *g, int precision, const void *d_app, const uint8_t *d_x,
                                const int32_t *d_it, int B, int k, int64_t *d_counts,
                                void *stream);
/* Bit errors (hard decision app < 0 against d_x, over all Nv bits) of each
 * codeword: d_bit_errors[B].  The per-codeword form lets a campaign stop at
 * the codeword where the frame-error count is reached (ldpc_awgn.py:86-105). */
int sg_ldpc_codeword_errors_device(sg_graph *g, int precision, const void *d_app, const uint8_t *d_x, int B,
                                   int32_t *d_bit_errors, void *stream);

/* ------------------------------------------- device encoder and channel */
/* Throughput-mode generation, keyed by Philox4x32-10
 * counters (seed, stream_id, codeword index, element): results depend only on
 * the key, not on B, the grid or the rank.  Parity mode (the reference's
 * numpy generators, seed for seed) stays on the host. */
/* nbits random bits per row, d_bits [B][nbits] uint8 (ldpc_awgn.py:44 / sparc.py:174-180) */
int sg_rng_bits_device(uint64_t seed, uint64_t stream_id, int B, int nbits, uint8_t *d_bits, void *stream);
/* section indices from MSB-first bit groups (sparc.py:330-364): d_bits [B][L*logM] -> d_idx [B][L] */
int sg_bits_to_sections_device(const uint8_t *d_bits, int B, int L, int logM, int32_t *d_idx, void *stream);
/* The same with row strides: codeword b's bits at d_bits + b * bit_stride,
 * its L indices at d_idx + b * idx_stride (a part of a longer message, e.g.
 * the protected sections of a concatenated codeword, sparc_new.py:15-51). */
int sg_bits_to_sections_strided_device(const uint8_t *d_bits, size_t bit_stride, int B, int L, int logM,
                                       int32_t *d_idx, size_t idx_stride, void *stream);
/* y = x + sigma N(0, 1) [B][n] (sparc_sim.py:179-204) */
int sg_awgn_device(int precision, uint64_t seed, uint64_t stream_id, const void *d_x, int B, int n, double sigma,
                   void *d_y, void *stream);
/* BPSK 1 - 2c over AWGN with variance sigma2, channel LLRs 2y/sigma2 [B][N] (ldpc_awgn.py:39-56) */
int sg_bpsk_awgn_llr_device(int precision, uint64_t seed, uint64_t stream_id, const uint8_t *d_cw, int B, int N,
                            double sigma2, void *d_llr, void *stream);
/* Systematic LDPC encoder (ldpc.py:400-460) as a GF(2) product: parity
 * [K][N-K] uint8 is the parity part of the code's generator (the encoder's
 * image of the unit vectors); cw = [info, info P]. */
typedef struct sg_ldpc_encoder sg_ldpc_encoder;
int sg_ldpc_encoder_create(const uint8_t *parity, int K, int N, sg_ldpc_encoder **out);
int sg_ldpc_encoder_destroy(sg_ldpc_encoder *e);
int sg_ldpc_encode_device(sg_ldpc_encoder *e, const uint8_t *d_info, int B, uint8_t *d_cw, void *stream);

/* ------------------------------------------------------ state evolution */
/* SPARC state evolution (sparc_public/sparc_se.py:82-183): Monte-Carlo samples
 * u [mc][M] (the reference's np.random.randn draw) stay on the device;
 * sg_se_expectation evaluates sparc_se_E (:82-115) for nt values of tau at
 * once (K = 1, or K = 2 for real modulated SPARCs).  Complex K-PSK SPARCs,
 * K = 4 .. 64 (a power of two; larger: SG_ERR_UNSUPPORTED), take complex
 * samples u [mc][M] interleaved double[2] (the reference's randn + 1j randn,
 * :154-155) from sg_se_samples_create_complex: K = 4 is the closed form in
 * sinh / cosh of the real and imaginary parts (:95-98), K >= 8 the mean over
 * the constellation of exp(Re(. conj c_k)) (:99-111), evaluated with the
 * section's largest exponent subtracted -- the same quantity wherever the
 * reference's unguarded exp is finite.  K >= 4 on real samples and K <= 2 on
 * complex samples are SG_ERR_INVALID. */
typedef struct sg_se_samples sg_se_samples;
int sg_se_samples_create(const double *u, int mc, int M, sg_se_samples **out);
int sg_se_samples_create_complex(const double *u, int mc, int M, sg_se_samples **out);
int sg_se_samples_destroy(sg_se_samples *h);
int sg_se_expectation(sg_se_samples *h, int K, const double *taus, int nt, double *E);

/* ------------------------------------------------- integrated AMP <-> BP */
/* The integrated decoders of sparc_sophie/sparc_new.py on a dense design
 * plan and an LDPC graph; every L log2 M bits of a codeword are LDPC
 * protected (ldpc_bp asserts it, sparc_new.py:1171).  mode:
 *   SG_INT_NAIVE       naively_integrated_decoder :257-282
 *   SG_INT_NAIVE_POST  naively_integrated_decoder_posteriors :411-439
 *   SG_INT_DIFF        integrated_decoder :472-502 (differentiated eta :824-841)
 *   SG_INT_DIFF_POST   integrated_decoder_posteriors :675-705 (:843-869)
 * y [B][n] -> bits [B][(L log2 M / N) K] (app[:K] < 0 of the final decode,
 * bp_its_final iterations; bp_its per intermediate decode; the reference uses
 * 6 and 200, sumprod2).  tau2 [B][t_max] (optional) receives tau^2 of every
 * iteration. */
enum sg_integrated_mode { SG_INT_NAIVE = 0, SG_INT_NAIVE_POST = 1, SG_INT_DIFF = 2, SG_INT_DIFF_POST = 3 };
int sg_integrated_decode(sg_dense_plan *p, sg_graph *g, int mode, int K, const double *y, int B, int t_max,
                         int bp_its, int bp_its_final, uint8_t *bits, double *tau2);
int sg_integrated_decode_device(sg_dense_plan *p, sg_graph *g, int mode, int K, const void *d_y, int B,
                                int t_max, int bp_its, int bp_its_final, uint8_t *d_bits, double *d_tau2,
                                void *stream);
/* The soft-glue functions on host arrays, batched over B codewords:
 * bp_output_to_beta_estimate :1260-1279 (probs [B][L log2 M] -> beta [B][L M]),
 * update_using_bp_probs :1030-1038, differentiated_eta_calc(_posteriors)
 * :824-869 (tau2 [B]; gamma ignored unless posteriors). */
int sg_bp_output_to_beta(int precision, const double *probs, int B, int L, int M, double sqrt_nPl,
                         double *beta);
int sg_update_using_bp_probs(int precision, const double *gamma, const double *alpha, int B, int L, int M,
                             double sqrt_nPl, double *beta);
int sg_differentiated_eta(int precision, int posteriors, const double *beta, const double *gamma,
                          const double *alpha, const double *vk, const double *vk0, const double *tau2, int B,
                          int L, int M, double sqrt_nPl, double *out);

/* Reference-compatible scalar entry points: exact signatures of the ctypes
 * targets in ldpc.py:481-503 (c_ldpc.c:32,138,234,294,339) with Linux LP64
 * `long`.  Each call decodes one codeword on the GPU in double precision. */
int sumprod(double *ch, long *vdeg, long *cdeg, long *intrlv, int Nv, int Nc, int Nmsg,
            double *app, int max_itcount);
int sumprod2(double *ch, long *vdeg, long *cdeg, long *intrlv, int Nv, int Nc, int Nmsg,
             double *app, int max_itcount);
int minsum(double *ch, long *vdeg, long *cdeg, long *intrlv, int Nv, int Nc, int Nmsg,
           double *app, double correction_factor, int max_itcount);
double Lxor(double L1, double L2, int corr_flag);
double Lxfb(double *L, long dc, int corr_flag);


/* -------------------------------------------------------------------- AMP */
typedef struct sg_amp_plan sg_amp_plan;

/* Design of a real SPARC with sub-sampled DCT operator (sparc.py:703-880):
 * base matrix W (ndim 0: scalar P; 1: power allocation vector of Lc blocks;
 * 2: spatially coupled Lr x Lc matrix), one transform per nonzero entry of W
 * in row-major order, whose row/column orders are order0[t][Mr] and
 * order1[t][Mc] exactly as generate_ordering (sparc.py:735-775) draws them
 * (Mr = n or n/Lr, Mc = L*M/Lc).  precision SG_F64 follows the reference's
 * double arithmetic; SG_F32 is the throughput path.  A plan eligible for the
 * per-codeword engine also holds a staged-engine plan at P = 16384, which
 * decodes batches too small for the per-codeword engine (sg_amp_plan_info
 * reports the per-codeword plan's P).  Section sizes: the regular engine
 * (ndim 0 or 1) takes any power of two M; a design that runs the general
 * engine (ndim 2 outside the block engines' geometries) with M > 2048 is
 * SG_ERR_UNSUPPORTED here, with no plan returned, never at decode time. */
int sg_amp_plan_create(int ndim, const double *W, int Lr, int Lc, int L, int M, int n,
                       const uint32_t *order0, const uint32_t *order1, int precision,
                       sg_amp_plan **out);
int sg_amp_plan_destroy(sg_amp_plan *p);
int sg_amp_plan_info(const sg_amp_plan *p, int *w, int *nT, int *Mr, int *Mc, int *P, int *Q);
/* Engine a decode of B codewords with this plan runs on: 0 general four-step
 * (amp_dct.hip), 1 staged regular (amp_fused.hip), 2 per-codeword
 * (amp_cw.hip), 3 block (amp_block.hip).  Reads SG_AMP_ENGINE like the
 * decoder; returns the engine or a negative error code. */
int sg_amp_plan_engine(const sg_amp_plan *p, int B);
/* What the last decode through this plan ran: *engine as sg_amp_plan_engine
 * (-1 before any decode and after a decode call with B = 0 or one that failed
 * before choosing an engine: every decode call resets it), *handover_iter the first iteration the per-codeword
 * engine left to the staged engine (-1: no hand-over), *on_companion 1 when
 * the decode ran on the P = 16384 companion plan (may be NULL). */
int sg_amp_last_decode(const sg_amp_plan *p, int *engine, int *handover_iter, int *on_companion);
/* The CU count the engine choice of this plan's decodes assumes instead of the device's (0: the device's): with
 * cus = 1 every batch runs the per-codeword engines, and the f32 split engine pipelines every batch of two or
 * more codewords.  For tests of the full-batch paths at small B. */
int sg_amp_plan_set_cus(sg_amp_plan *p, int cus);
/* *pipelined 1 when the last decode through this plan ran split-engine iterations as two half-batches on two
 * streams (B >= the CU count and at least 2; SG_AMP_PIPE=0 keeps one stream). */
int sg_amp_last_pipelined(const sg_amp_plan *p, int *pipelined);

/* Batched AMP decode (sparc.py:883-999, one call per codeword in the
 * reference): y[B][n] received words sharing the plan's design; true_idx
 * [B][L] (optional) the transmitted section indices, used for NMSE.
 * Outputs: map_idx[B][L] final MAP section indices (argmax of s, sparc.py:997),
 * t_final[B], nmse[B][t_max][Lc], psi[B][Lc] (sparc.py:999 return values). */
int sg_amp_decode(sg_amp_plan *p, const double *y, int B, const int32_t *true_idx, double awgn_var,
                  int t_max, double rtol, int phi_method, int32_t *map_idx, int32_t *t_final,
                  double *nmse, double *psi);
/* Device variant: d_y in the plan precision (float or double), all outputs
 * device-resident (any output may be NULL). */
int sg_amp_decode_device(sg_amp_plan *p, const void *d_y, int B, const int32_t *d_true_idx,
                         double awgn_var, int t_max, double rtol, int phi_method,
                         int32_t *d_map_idx, int32_t *d_t_final, double *d_nmse, double *d_psi,
                         void *stream);
/* AMP with known sections (amp_oploop.hip): sg_amp_decode_device's loop (sparc.py:883-999) in which some
 * sections of a codeword are given.  d_known_idx [B][L] holds a section's index in [0, M), or -1 for a section
 * to decode; the known set is per codeword.  The denoiser of a known section returns the one-hot of its index (it
 * adds 1 to sum beta^2, 0 to psi, and 0 to the NMSE where it agrees with d_true_idx); the start is beta0 = the
 * known one-hots, z0 = y - Ab(beta0), psi0_c = the share of unknown sections of column block c, so gamma0 = W psi0
 * (flat) or dot(W, psi0) / Lc (power allocation), and iteration 0 has no Onsager term.  Everything else -- phi by
 * either phi_method, tau, s = beta + tau Az(z / phi), the psi stopping rule, the final MAP on s -- is the
 * reference loop; a known section reports its known index in d_map_idx.  With every entry -1 this is
 * sg_amp_decode_device's arithmetic.  Outputs as there (any may be NULL).  Every check precedes any launch or
 * allocation: SG_ERR_UNSUPPORTED for a spatially coupled plan (W of ndim 2) and for M not a power of two in
 * [2, 2048] (one wavefront per section, up to 32 entries per lane); SG_ERR_INVALID for bad t_max, rtol,
 * phi_method, awgn_var as sg_amp_decode_device; B <= 0 returns SG_OK with nothing done.  The device variant treats
 * a known index outside [-1, M) as unknown.  Works in the plan's workspace on the plan's own operators (never the
 * companion plan): clears the last-decode state (a following sg_amp_llr* answers SG_ERR_BAD_ARG, as after
 * sg_amp_apply*) and leaves the plan fit for sg_amp_decode*.  The partial buffers are allocated once per
 * (plan, B) and freed with the plan; the loop itself enqueues on the stream and polls the active flags as
 * sg_amp_decode_device does.  A codeword's results do not depend on the batch it is decoded in. */
int sg_amp_decode_partial_device(sg_amp_plan *p, const void *d_y, int B, const int32_t *d_known_idx,
                                 const int32_t *d_true_idx, double awgn_var, int t_max, double rtol,
                                 int phi_method, int32_t *d_map_idx, int32_t *d_t_final, double *d_nmse,
                                 double *d_psi, void *stream);
/* Host variant: arrays as sg_amp_decode plus known_idx [B][L]; blocking.  It scans known_idx: an entry outside
 * [-1, M) is SG_ERR_INVALID, before anything is launched. */
int sg_amp_decode_partial(sg_amp_plan *p, const double *y, int B, const int32_t *known_idx,
                          const int32_t *true_idx, double awgn_var, int t_max, double rtol, int phi_method,
                          int32_t *map_idx, int32_t *t_final, double *nmse, double *psi);
/* Real K = 2 (BPSK) modulated SPARCs (amp_oploop.hip): sg_amp_decode_device's loop (sparc.py:883-999) with the
 * non-zero entry of a section +1 or -1.  A section is one word = (location << 1) | symbol in [0, 2M), symbol 0 for
 * +1 and 1 for -1: its binary digits, MSB first, are the section's log2 M location bits and its one symbol bit in
 * the reference's order (sparc.py:330-364), so sg_bits_to_sections_device and sg_amp_count_errors_device serve K = 2
 * with logM + 1 in the place of logM.  d_true_word [B][L] (optional) gives the transmitted words, for the NMSE
 * against the +-1 one-hots.  The denoiser is beta_j = (e^{x_j} - e^{-x_j}) / sum_k (e^{x_k} + e^{-x_k}), x = s / tau
 * (sparc.py:433-441), evaluated with the section's own maximum of |x| and expm1; everything else -- gamma, the
 * Onsager term, phi by either phi_method, tau, psi = 1 - |beta|^2 / L per column block, the psi stopping rule --
 * is the unmodulated loop.  d_map_word [B][L] is the final decision on s (sparc.py:488-492): the first location
 * of the largest |s| and the sign of s there (+1 for s >= 0).  Other outputs as sg_amp_decode_device (any may be
 * NULL).  Serves every plan sg_amp_apply serves -- flat, power-allocated and spatially coupled W, both precisions
 * -- on the plan's own operators (never the companion plan, no throughput engine).  Every check precedes any
 * launch or allocation: SG_ERR_UNSUPPORTED for M not a power of two in [2, 2048] (one wavefront per section, up to
 * 32 entries per lane); SG_ERR_INVALID for bad t_max, rtol, phi_method, awgn_var as sg_amp_decode_device; B <= 0
 * returns SG_OK with nothing done.  Works in the workspace and the partial buffers of sg_amp_decode_partial_device:
 * clears the last-decode state (sg_amp_llr* refuses after a K = 2 decode; its soft output is sg_amp_bpsk_llr*
 * below) and leaves the plan fit for sg_amp_decode*.  A codeword's results do not depend on the batch it is
 * decoded in. */
int sg_amp_decode_bpsk_device(sg_amp_plan *p, const void *d_y, int B, const int32_t *d_true_word, double awgn_var,
                              int t_max, double rtol, int phi_method, int32_t *d_map_word, int32_t *d_t_final,
                              double *d_nmse, double *d_psi, void *stream);
/* Host variant: arrays as sg_amp_decode with words in the place of indices; blocking. */
int sg_amp_decode_bpsk(sg_amp_plan *p, const double *y, int B, const int32_t *true_word, double awgn_var, int t_max,
                       double rtol, int phi_method, int32_t *map_word, int32_t *t_final, double *nmse, double *psi);
/* Real K = 2 AMP with known section words (amp_oploop.hip): sg_amp_decode_bpsk_device's loop in which some sections
 * of a codeword are given, the final pass of the three-stage K = 2 decoder.  d_known_word [B][L] holds a section's
 * word (location << 1) | symbol in [0, 2M) -- what sg_concat_known_sections_device writes at log2 M + 1 bits per
 * section -- or -1 for a section to decode; the known set is per codeword.  The denoiser of a known section returns
 * the +-1 one-hot of its word: +1 (symbol 0) or -1 at the location.  It adds 1 to sum beta^2, 0 to psi, and to the
 * section's squared error against d_true_word 0 where the words agree, 4 at the same location with the opposite
 * sign, 2 at another location, 1 without a true word.  The start is beta0 = the known one-hots, z0 = y - Ab(beta0),
 * psi0_c = the share of unknown sections of column block c, gamma0 from psi0, no Onsager term in iteration 0;
 * everything else is sg_amp_decode_bpsk_device's loop, and a known section reports its known word in d_map_word.
 * With every entry -1 the outputs are sg_amp_decode_bpsk_device's, bit for bit.  Flat, power-allocated and spatially
 * coupled W, both precisions.  Refusals as sg_amp_decode_bpsk_device, all before any launch or allocation; the device
 * variant treats a word outside [0, 2M) as unknown.  A decode with known words keeps no soft state, whatever
 * sg_amp_bpsk_soft_output says: s is not stored and sg_amp_bpsk_llr* refuses afterwards, until the next
 * sg_amp_decode_bpsk*.  A codeword's results do not depend on the batch it is decoded in. */
int sg_amp_decode_bpsk_partial_device(sg_amp_plan *p, const void *d_y, int B, const int32_t *d_known_word,
                                      const int32_t *d_true_word, double awgn_var, int t_max, double rtol,
                                      int phi_method, int32_t *d_map_word, int32_t *d_t_final, double *d_nmse,
                                      double *d_psi, void *stream);
/* Host variant: arrays as sg_amp_decode_bpsk plus known_word [B][L]; blocking.  It scans known_word: an entry
 * outside [-1, 2M) is SG_ERR_BAD_ARG naming its index, before anything is launched. */
int sg_amp_decode_bpsk_partial(sg_amp_plan *p, const double *y, int B, const int32_t *known_word,
                               const int32_t *true_word, double awgn_var, int t_max, double rtol, int phi_method,
                               int32_t *map_word, int32_t *t_final, double *nmse, double *psi);
/* x = A beta0 [B][n] on the device for section words d_word [B][L] of a real K = 2 SPARC: beta0 holds +1
 * (symbol 0) or -1 at the word's location; a word outside [0, 2M) leaves its section zero. */
int sg_amp_encode_bpsk_device(sg_amp_plan *p, const int32_t *d_word, int B, void *d_x, void *stream);
/* Soft output of the K = 2 decoder (amp_bpsk_llr.hip).  The decoder overwrites beta in place, so the bit
 * marginals need the last effective observation s = beta + tau u of each codeword.  sg_amp_bpsk_soft_output(p, 1)
 * makes the following sg_amp_decode_bpsk* through this plan keep it: sizeof(real) L M bytes per codeword of the
 * batch, allocated with the operator loop's buffers on the next K = 2 decode (grow-only, freed with the plan); off
 * (the default) nothing is allocated and nothing is stored.  map_word, t_final, nmse and psi are the same bits
 * either way.  Switching clears the state below. */
int sg_amp_bpsk_soft_output(sg_amp_plan *p, int on);
/* For sections [l0, l0 + nl) of each of the B codewords of the last K = 2 decode through this plan, in the plan
 * precision: P(bit = 0) of the log2 M location bits, MSB first, and then of the symbol bit (0: +1) -- the digits
 * of the section's word -- under the joint posterior p(j, c) = e^{c x_j} / sum_k (e^{x_k} + e^{-x_k}), x = s / tau,
 * c = +-1, whose mean is the decoder's beta; clipped to [1e-15, 1 - 1e-15] and written as log p - log(1 - p)
 * (ldpc_bp, sparc_new.py:1167-1169) to d_llr[b * llr_ld + (l - l0) * (log2 M + 1) + i]; probs_only: the unclipped
 * probabilities.  A codeword that stopped early gives the s and the tau of its last executed iteration.  Enqueued
 * on the stream; allocates nothing; the same bits on every run, and a codeword's output does not depend on its
 * batch.  Every refusal precedes any launch or write.  SG_ERR_UNSUPPORTED: M not a power of two in [2, 2048].
 * SG_ERR_BAD_ARG: soft output off; no K = 2 decode with soft output on record (every decode call of any kind
 * through the plan, sg_amp_apply*, the encoders and the integrated decoders clear it; a failed or B = 0 decode
 * leaves it cleared); B different from that decode's; a section range outside [0, L]; llr_ld < nl (log2 M + 1). */
int sg_amp_bpsk_llr_device(sg_amp_plan *p, int B, int l0, int nl, int llr_ld, int probs_only, void *d_llr,
                           void *stream);
/* Host variant: out [B][nl * (log2 M + 1)] as double, blocking.  A decode enqueued on a caller's stream must have
 * completed. */
int sg_amp_bpsk_llr(sg_amp_plan *p, int B, int l0, int nl, int probs_only, double *out);
/* Soft output of the last decode through this plan (sg_amp_decode_device or
 * sg_amp_decode), in the plan precision: for sections [l0, l0 + nl) of each of
 * the B codewords, P(bit = 0) of the log2 M section bits, MSB first, from the
 * final beta = softmax(s / tau) (beta_estimate_to_bp_probs,
 * sparc_new.py:1118-1138), clipped to [1e-15, 1 - 1e-15] and written as
 * log p - log(1 - p) (ldpc_bp, :1167-1169) to d_llr[b * llr_ld + (l - l0) * log2 M + i];
 * probs_only: the unclipped probabilities themselves.  Enqueued on the
 * stream; reads the state the decode left in the plan (of the sub-plan that
 * ran, a codeword that stopped early with the tau of its last iteration) and
 * allocates nothing.  SG_ERR_BAD_ARG: no decode yet (every decode call resets
 * the state; sg_amp_apply*, sg_amp_encode_device overwrite it and clear it
 * too), B different from the decode's batch, a section range outside [0, L],
 * llr_ld < nl log2 M, M < 2 or not a power of two.  SG_ERR_UNSUPPORTED: plans
 * of the single-precision block engines (amp_block.hip, amp_block2.hip;
 * spatially coupled designs give soft output in double precision), M > 2048. */
int sg_amp_llr_device(sg_amp_plan *p, int B, int l0, int nl, int llr_ld, int probs_only, void *d_llr,
                      void *stream);
/* Host variant: out [B][nl * log2 M] as double, blocking.  A decode enqueued on a
 * caller's stream must have completed. */
int sg_amp_llr(sg_amp_plan *p, int B, int l0, int nl, int probs_only, double *out);
/* Design operators (the Ab / Az closures of sparc_transforms, sparc.py:786-875):
 * transpose 0: in[B][L*M] -> out[B][n];  transpose 1: in[B][n] -> out[B][L*M]. */
int sg_amp_apply(sg_amp_plan *p, int transpose, const double *in, int B, double *out);
/* x = A beta0 [B][n] on the device for section indices d_idx [B][L]
 * (one-hot beta0 with value 1, sparc.py:17-53 sparc_encode). */
int sg_amp_encode_device(sg_amp_plan *p, const int32_t *d_idx, int B, void *d_x, void *stream);
/* Diagnostics: mean shader-clock cycles of the phases of the last stage-1
 * launches (kernel 0 = Ab stage 1, 1 = Az stage 2; mean_cycles[8], entry k =
 * timestamp k minus timestamp k-1).  Only with SG_AMP_TPROF set in the
 * environment; otherwise *nphases = 0. */
int sg_amp_stage_profile(sg_amp_plan *p, int kernel, double *mean_cycles, int *nphases);
/* Diagnostics: the raw phase timestamps behind sg_amp_stage_profile, [items][10]:
 * 8 shader-clock values (per-XCD clocks) then the start and end on the 100 MHz
 * device-wide realtime clock, of the last iteration (items = B * column blocks * classes);
 * *items = 0 when SG_AMP_TPROF was not set.  out may be null to query *items. */
int sg_amp_stage_raw(sg_amp_plan *p, int kernel, uint64_t *out, size_t *items);
int sg_amp_apply_device(sg_amp_plan *p, int transpose, const void *d_in, int B, void *d_out,
                        void *stream);
/* Adds {section errors, bit errors (popcount of index XOR, MSB-first bits as
 * sparc.py:182-197), codeword errors, sum of t_final} into d_counts[4]. */
int sg_amp_count_errors_device(const int32_t *d_map_idx, const int32_t *d_true_idx,
                               const int32_t *d_t_final, int B, int L, int logM, int64_t *d_counts,
                               void *stream);

/* The four integrated AMP <-> BP decoders (enum sg_integrated_mode) on a sub-sampled DCT design plan
 * (integrated_dct.hip): the mathematics of
 * sg_integrated_decode with the design matrix replaced by the plan's operator, A beta -> Ab(beta) / snp and
 * A^T z -> Az(z) / snp, snp = sqrt(n P / L), P the plan's scalar W (that matrix is
 * A[i][j] = sqrt(2 / n) cos(pi (2 order1[j] + 1) order0[i] / (2 w))).  d_y in the plan precision; d_bits
 * [B][(L log2 M / N) K]; d_tau2 [B][t_max] optional; d_app optional: the final BP output [B L log2 M / N][N]
 * in the plan precision (for sg_concat_count_errors_device).  Intermediate and final BP run sumprod2.
 * Every check precedes any launch or allocation: SG_ERR_UNSUPPORTED for a plan that is not flat (W of ndim 1
 * or 2: the fork's decoders know one P_l and one tau^2) and for M not a power of two in [2, 2048] (the section
 * kernel's width); SG_ERR_INVALID for L log2 M not a multiple of N, K outside (0, N], bad iteration counts;
 * B <= 0 returns SG_OK with nothing done.  Works in the plan's workspace: clears the last-decode state (a
 * following sg_amp_llr* answers SG_ERR_BAD_ARG, as after sg_amp_apply*) and leaves the plan fit for
 * sg_amp_decode*.  The integrated buffers are allocated once per (plan, B) and freed with the plan; the loop
 * itself enqueues on the stream without synchronising. */
int sg_amp_integrated_decode_device(sg_amp_plan *p, sg_graph *g, int mode, int K, const void *d_y, int B,
                                    int t_max, int bp_its, int bp_its_final, uint8_t *d_bits, void *d_app,
                                    double *d_tau2, void *stream);
/* Host variant: y [B][n], bits and tau2 (optional) as sg_integrated_decode; blocking. */
int sg_amp_integrated_decode(sg_amp_plan *p, sg_graph *g, int mode, int K, const double *y, int B, int t_max,
                             int bp_its, int bp_its_final, uint8_t *bits, double *tau2);

/* Stand-alone section estimators, double precision on the GPU:
 * out[l*M+j] = scale * softmax_j(x[l*M : (l+1)*M])  (msg_vector_mmse_estimator,
 * sparc.py:429-432 / sparc_new.py:1058-1066 with x = s/tau);
 * idx[l] = argmax_j s[l*M+j], first maximum (msg_vector_map_estimator, sparc.py:485-487). */
int sg_section_softmax(const double *x, int L, int M, double scale, double *out);
int sg_section_argmax(const double *x, int L, int M, int32_t *idx);

/* ------------------------------------------------- complex / K-PSK AMP */
typedef struct sg_camp_plan sg_camp_plan;

/* Design of a complex SPARC with sub-sampled FFT operator (sparc.py:593-646,
 * 703-880 with csparc=True): W, L, M, n and the transforms as sg_amp_plan_create;
 * order0[t][Mr] / order1[t][Mc] index the bins of a w-point FFT,
 * w = 2^ceil(log2(max(Mr+2, Mc+2))), 16 <= w <= 2^20 (SG_ERR_UNSUPPORTED
 * otherwise).  Double precision only.  Complex arrays cross this ABI as
 * interleaved double[2] (re, im).  The workspace holds two buffers of
 * 16 nT w bytes per codeword (32 MB per transform at w = 2^20).
 * sg_camp_plan_info: P and Q are the two factors of the transform's
 * four-step split, w = P Q: P = 2^floor(log2 w / 2) up to w = 2^16, P = 256
 * above. */
int sg_camp_plan_create(int ndim, const double *W, int Lr, int Lc, int L, int M, int n,
                        const uint32_t *order0, const uint32_t *order1, sg_camp_plan **out);
int sg_camp_plan_destroy(sg_camp_plan *p);
int sg_camp_plan_info(const sg_camp_plan *p, int *w, int *nT, int *Mr, int *Mc, int *P, int *Q);
/* transpose 0: A x, in[B][L*M] -> out[B][n];  transpose 1: A^H y, in[B][n] -> out[B][L*M]
 * (the Ab / Az closures of sparc_transforms(..., csparc=True)). */
int sg_camp_apply(sg_camp_plan *p, int transpose, const double *in, int B, double *out);
/* Batched AMP decode of complex received words y[B][n] (sparc.py:883-999).
 * K = 1: unmodulated; K = 2 .. 64 (a power of two; larger: SG_ERR_UNSUPPORTED):
 * K-PSK with the host's constellation constel[K] (psk_constel, sparc.py:225-239).
 * true_idx / true_sym [B][L] (optional): the transmitted locations and
 * constellation indices, used for NMSE.  Outputs: map_idx / map_sym [B][L] the
 * MAP location and constellation index of the last s (sparc.py:997), t_final[B],
 * nmse[B][t_max][Lc], psi[B][Lc].  The *_sym arrays are ignored (may be NULL)
 * for K = 1. */
int sg_camp_decode(sg_camp_plan *p, const double *y, int B, int K, const double *constel,
                   const int32_t *true_idx, const int32_t *true_sym, double awgn_var, int t_max,
                   double rtol, int phi_method, int32_t *map_idx, int32_t *map_sym,
                   int32_t *t_final, double *nmse, double *psi);
/* Device variant (sg_camp_decode is upload -> this -> download): d_y [B][n]
 * interleaved complex, only read; every d_* output may be NULL.  constel stays
 * a host array.  The checks of sg_camp_decode apply except the range scan of
 * the true indices: d_true_idx must lie in [0, M) and d_true_sym in [0, K).
 * The decoder's state lives in the plan, so one call at a time per plan; the
 * host polls the codewords' `active` flags every four iterations (the only
 * synchronisation), otherwise the call returns without synchronising. */
int sg_camp_decode_device(sg_camp_plan *p, const void *d_y, int B, int K, const double *constel,
                          const int32_t *d_true_idx, const int32_t *d_true_sym, double awgn_var, int t_max,
                          double rtol, int phi_method, int32_t *d_map_idx, int32_t *d_map_sym,
                          int32_t *d_t_final, double *d_nmse, double *d_psi, void *stream);

/* Device-resident Monte-Carlo campaign of a complex / K-PSK SPARC (all d_*
 * device pointers; Philox generation as "device encoder and channel" above):
 *   sg_rng_bits_device               B x L (logM + logK) message bits
 *   sg_bits_to_psk_sections_device   bits -> location and constellation index
 *   sg_camp_encode_device            x = A beta0
 *   sg_awgn_device                   complex AWGN of variance awgn_var is
 *       sg_awgn_device(SG_F64, seed, stream_id, d_x, B, 2 * n, sqrt(awgn_var / 2),
 *       d_y, stream) on the interleaved reals (sparc_sim.py:179-204, complex
 *       branch): there is no complex noise entry point
 *   sg_camp_decode_device            AMP
 *   sg_camp_count_errors_device      error counters. */
/* d_bits [B][L*(logM+logK)] uint8 -> per section the location d_idx [B][L] from
 * logM MSB-first bits and the constellation index d_sym [B][L] = gray2bin of
 * the following logK Gray-coded PSK bits (bin_arr_2_msg_vector, sparc.py:330-364).
 * logK = 0 (K = 1): d_sym may be NULL, and is written as zero otherwise. */
int sg_bits_to_psk_sections_device(const uint8_t *d_bits, int B, int L, int logM, int logK, int32_t *d_idx,
                                   int32_t *d_sym, void *stream);
/* x = A beta0 [B][n] interleaved complex, beta0 with constel[d_sym] (1 for
 * K = 1, where constel and d_sym may be NULL) at location d_idx of every
 * section (sparc.py:17-53 sparc_encode); constel is the host's psk_constel(K)
 * as for sg_camp_decode.  A location outside [0, M) or a constellation index
 * outside [0, K) leaves its section empty. */
int sg_camp_encode_device(sg_camp_plan *p, int K, const double *constel, const int32_t *d_idx,
                          const int32_t *d_sym, int B, void *d_x, void *stream);
/* Adds {section errors, location errors, value errors, bit errors, codeword
 * errors, sum of t_final} into int64 d_counts[6]; if d_rows is not NULL also
 * writes int32 d_rows[B][4] = {bit, section, location, value errors} of each
 * codeword.  As calc_ler_ver (sparc_sim.py:100-175) and calc_ber over
 * msg_vector_2_bin_arr (sparc.py:366-400): location error = locations differ;
 * value error = constellation indices differ, wherever the location is;
 * section error = either; bit errors = popcount(idx ^ idx') +
 * popcount(gray(sym) ^ gray(sym')); codeword error = any bit error.
 * logK = 0: the *_sym pointers are ignored (may be NULL). */
int sg_camp_count_errors_device(const int32_t *d_map_idx, const int32_t *d_map_sym, const int32_t *d_true_idx,
                                const int32_t *d_true_sym, const int32_t *d_t_final, int B, int L, int logM,
                                int logK, int64_t *d_counts, int32_t *d_rows, void *stream);
/* Stand-alone K-PSK section estimators (sparc.py:402-512).  x = s / tau with
 * tau already halved for complex s, [L*M] interleaved complex if x_is_complex
 * else real; out[L*M] interleaved complex (imaginary part 0 for K <= 2). */
int sg_section_mmse_psk(const double *x, int L, int M, int K, const double *constel,
                        int x_is_complex, double *out);
/* idx[l] the MAP location of section l, sym[l] its constellation index (0 for
 * K = 1, where sym may be NULL); first maximum in row-major order. */
int sg_section_map_psk(const double *s, int L, int M, int K, const double *constel,
                       int s_is_complex, int32_t *idx, int32_t *sym);

/* Soft output of the complex engine (camp_llr.hip).  A section carries
 * log2 M MSB-first location bits, then log2 K Gray-coded K-PSK bits
 * (msg_vector_2_bin_arr, sparc.py:366-400).  For K >= 2 the decoder's final
 * beta is a conditional mean, not a posterior, so P(bit = 0) is a marginal of
 * the joint posterior p(j, k) ~ exp(Re(x_j conj c_k)), x = s / (tau / 2), of
 * the last effective observation s = beta + tau u and its tau.
 * sg_camp_soft_output(p, 1) makes the following decodes keep that s: 16 L M
 * bytes per codeword, allocated with the batch workspace on the next decode;
 * off (the default) nothing is allocated and the decoder stores what it always
 * did.  Switching clears the state below. */
int sg_camp_soft_output(sg_camp_plan *p, int on);
/* For sections [l0, l0 + nl) of each of the B codewords of the last decode
 * through this plan: P(bit = 0) of the log2 M + log2 K section bits, clipped
 * to [1e-15, 1 - 1e-15] and written as log p - log(1 - p) (ldpc_bp,
 * sparc_new.py:1167-1169) to d_llr[b * llr_ld + (l - l0) * (log2 M + log2 K) + i];
 * probs_only: the unclipped probabilities.  A codeword that stopped early
 * gives the s and the tau of its last executed iteration.  K and constel as
 * the decode's.  Enqueued on the stream; allocates nothing.  SG_ERR_BAD_ARG:
 * soft output off; no decode yet, or its state cleared (every decode call
 * resets it, a failed or B = 0 one leaves it cleared; sg_camp_apply and
 * sg_camp_encode_device clear it); B or K different from the decode's; a
 * section range outside [0, L]; llr_ld < nl (log2 M + log2 K); M < 2.
 * SG_ERR_UNSUPPORTED: M > 2048. */
int sg_camp_llr_device(sg_camp_plan *p, int B, int K, const double *constel, int l0, int nl, int llr_ld,
                       int probs_only, double *d_llr, void *stream);
/* Host variant: out [B][nl * (log2 M + log2 K)], blocking.  A decode enqueued
 * on a caller's stream must have completed. */
int sg_camp_llr(sg_camp_plan *p, int B, int K, const double *constel, int l0, int nl, int probs_only,
                double *out);
/* The same function of a caller's vector, the twin of sg_section_mmse_psk:
 * x = s / tau with tau already halved, [L*M] interleaved complex if
 * x_is_complex else real (K <= 2: the exponents are +-x); out
 * [L][log2 M + log2 K].  M a power of two in [2, 2048] (larger:
 * SG_ERR_UNSUPPORTED). */
int sg_section_llr_psk(const double *x, int L, int M, int K, const double *constel, int x_is_complex,
                       int probs_only, double *out);
/* sg_bits_to_psk_sections_device with row strides, as
 * sg_bits_to_sections_strided_device: codeword b's L (logM + logK) bits at
 * d_bits + b * bit_stride, its L locations and constellation indices at
 * d_idx / d_sym + b * idx_stride. */
int sg_bits_to_psk_sections_strided_device(const uint8_t *d_bits, size_t bit_stride, int B, int L, int logM,
                                           int logK, int32_t *d_idx, int32_t *d_sym, size_t idx_stride,
                                           void *stream);
/* d_word [B][L] = d_idx << logK | bin2gray(d_sym): the log2 M + log2 K message
 * bits of every section as one integer (logK = 0: d_sym may be NULL), so that
 * sg_concat_count_errors_device counts a K-PSK codeword's unprotected bits
 * with logM + logK in the place of logM. */
int sg_psk_pack_sections_device(const int32_t *d_idx, const int32_t *d_sym, int B, int L, int logK,
                                int32_t *d_word, void *stream);
/* Its inverse: a word < 0 gives d_idx = -1 and d_sym = 0 (the "unknown" of
 * sg_concat_known_sections_device), any other d_idx = word >> logK and
 * d_sym = gray2bin(word & (K - 1)).  logK = 0: d_sym may be NULL, and is
 * written as zero otherwise. */
int sg_psk_unpack_sections_device(const int32_t *d_word, int B, int L, int logK, int32_t *d_idx, int32_t *d_sym,
                                  void *stream);

/* Complex AMP with known sections: sg_camp_decode_device with some sections of
 * each codeword given (the final pass of the three-stage concatenated K-PSK
 * decoder AMP -> BP -> AMP).  d_known_idx [B][L] holds a section's location in
 * [0, M), or -1 for a section to decode; d_known_sym [B][L] its constellation
 * index in [0, K) (may be NULL for K = 1); the set is per codeword.  A known
 * section's estimate is the one-hot c[sym] at idx throughout: it adds 1 to sum
 * |beta|^2 (0 to psi), and 0 to the NMSE where (idx, sym) agrees with
 * d_true_idx / d_true_sym.  The start is beta0 = the known one-hots,
 * z0 = y - Ab(beta0), psi0_c = the share of unknown sections of column block
 * c, gamma0 formed from psi0 as the loop forms gamma from psi (W psi for ndim
 * 0, dot(W, psi) / Lc otherwise), and iteration 0 has no Onsager term.
 * Everything else -- phi by either phi_method, tau, s = beta + tau Az(z / phi),
 * the K-PSK MMSE estimate of an unknown section, the psi stopping rule, the
 * final MAP of s -- is sg_camp_decode_device's, for W of ndim 0, 1 and 2 and
 * any M it takes; d_map_idx / d_map_sym report the known (idx, sym) of a known
 * section.  With every entry -1 this is sg_camp_decode_device's arithmetic.
 * Outputs as there (any may be NULL).
 *   Every check precedes any launch or allocation and is
 * sg_camp_decode_device's: SG_ERR_INVALID for bad t_max, rtol, phi_method,
 * awgn_var, K, B > 65535, a NULL d_known_idx, or K > 1 with a NULL
 * d_known_sym; SG_ERR_UNSUPPORTED for K > 64; B <= 0 returns SG_OK with
 * nothing done.  The device variant treats a location outside [0, M) as
 * unknown and reduces d_known_sym modulo K.
 *   Works in the plan's workspace: clears the last-decode state (a following
 * sg_camp_llr* answers SG_ERR_BAD_ARG; the soft-output buffer is not written)
 * and leaves the plan fit for sg_camp_decode*.  The loop enqueues on the
 * stream and polls the active flags as sg_camp_decode_device does.  A
 * codeword's results do not depend on the batch it is decoded in. */
int sg_camp_decode_partial_device(sg_camp_plan *p, const void *d_y, int B, int K, const double *constel,
                                  const int32_t *d_known_idx, const int32_t *d_known_sym,
                                  const int32_t *d_true_idx, const int32_t *d_true_sym, double awgn_var,
                                  int t_max, double rtol, int phi_method, int32_t *d_map_idx,
                                  int32_t *d_map_sym, int32_t *d_t_final, double *d_nmse, double *d_psi,
                                  void *stream);
/* Host variant: arrays as sg_camp_decode plus known_idx / known_sym [B][L];
 * blocking.  It scans them: a known_idx outside [-1, M), or a known_sym outside
 * [0, K) on a known section, is SG_ERR_INVALID before anything is launched.
 * The device copies of the known arrays are allocated once per (plan, B) and
 * freed with the plan. */
int sg_camp_decode_partial(sg_camp_plan *p, const double *y, int B, int K, const double *constel,
                           const int32_t *known_idx, const int32_t *known_sym, const int32_t *true_idx,
                           const int32_t *true_sym, double awgn_var, int t_max, double rtol, int phi_method,
                           int32_t *map_idx, int32_t *map_sym, int32_t *t_final, double *nmse, double *psi);

#ifdef __cplusplus
}
#endif
#endif /* LDPC_SPARC_AMD_H */
