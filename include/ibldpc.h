/*
 * ibldpc.h — C ABI of the MI355X-native batched LDPC decoding engine (libibldpc.so).
 *
 * Drop-in boundary for the reference's decoder classes (mx-strk/InformationBottleneckDecodingLDPC,
 * snapshot 2024-10-22).  Each entry point names the reference interface it replaces; the
 * Python classes in informationbottleneckdecodingldpc_amd/ keep the reference's method
 * names and call these through ctypes.
 *
 * Conventions
 *   - return 0 (IBL_OK) or a negative IBL_E* code; the message of the last failure on the
 *     calling thread is returned by ibl_last_error();
 *   - d_* pointers are DEVICE pointers owned by the caller (e.g. torch ROCm tensors'
 *     data_ptr() or hipMalloc); `stream` is a hipStream_t (NULL = default stream);
 *   - decode calls are asynchronous on `stream` and never synchronise the host
 *     (the reference reads the syndrome back every iteration; here the early stop is
 *     decided on the device);
 *   - a handle owns its device tables and scratch, is bound to the device it was created
 *     on and is not thread-safe (as the reference's decoder objects, which own their inboxes);
 *   - arrays are [row][codeword] with row stride B (the reference's received_blocks layout).
 */
#ifndef IBLDPC_H
#define IBLDPC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IBL_VERSION 3

enum { IBL_OK = 0, IBL_EINVAL = -1, IBL_EHIP = -2, IBL_ENOMEM = -3, IBL_EUNSUPPORTED = -4 };
enum { IBL_U8 = 1, IBL_I32 = 2, IBL_F32 = 3, IBL_F64 = 4, IBL_I8 = 5 };   /* IBL_I8: fixed-point layered only */
enum { IBL_MINSUM = 0, IBL_BP = 1 };
enum { IBL_PATH_AUTO = 0, IBL_PATH_PASSES = 1, IBL_PATH_FUSED = 2 };
enum { IBL_FLAG_FORCE_GENERIC = 1 };

typedef struct ibl_graph ibl_graph;
typedef struct ibl_ib ibl_ib;
typedef struct ibl_float ibl_float;

int ibl_version(void);
const char* ibl_last_error(void);
/* number of visible HIP devices (0 on a machine without GPU) */
int ibl_device_count(int32_t* n);

/*
 * Tanner-graph index construction on the HOST (no device needed).
 * Replaces map_node_connections (Discrete_LDPC_decoding/discrete_LDPC_decoder_irreg.py:121-170;
 * regular copy discrete_LDPC_decoder.py:88-130).  Input: canonical CSR of H (column indices
 * strictly ascending within each row).  Outputs (caller-allocated): cn_start[n_c], cn_deg[n_c],
 * tgt_cn[E] (= target_memory_cells_checknodes), vn_start[n_v], vn_deg[n_v],
 * tgt_vn[E] (= target_memory_cells_varnodes).
 */
int ibl_map_node_connections(int32_t n_v, int32_t n_c, const int32_t* csr_indptr, const int32_t* csr_cols,
                             int32_t* cn_start, int32_t* cn_deg, int32_t* tgt_cn,
                             int32_t* vn_start, int32_t* vn_deg, int32_t* tgt_vn);

/*
 * Upload a code graph to `device` (host arrays in, canonical CSR of H).
 * Replaces the index-array upload half of init_OpenCL_decoding
 * (discrete_LDPC_decoder_irreg.py:191-204, min_sum_decoder_irreg.py:182-195).
 */
int ibl_graph_create(int32_t n_v, int32_t n_c, const int32_t* csr_indptr, const int32_t* csr_cols,
                     int32_t device, ibl_graph** out);
int ibl_graph_info(const ibl_graph* g, int32_t* n_v, int32_t* n_c, int64_t* n_e, int32_t* d_c_max,
                   int32_t* d_v_max);
void ibl_graph_destroy(ibl_graph* g);

/*
 * Information-bottleneck (integer lookup-table) decoder.
 * Replaces Discrete_LDPC_Decoder_class_irregular.init_OpenCL_decoding
 * (discrete_LDPC_decoder_irreg.py:172-243) and Discrete_LDPC_Decoder_class.init_OpenCL_decoding
 * (discrete_LDPC_decoder.py:132-200): uploads the CN / VN LUT vectors (reference layout, int32,
 * entries in [0, T_dec)), the matching vectors (irregular class; ignored unless match != 0) and
 * allocates inboxes for up to max_batch codewords (`msg_at_time`).  The CN/VN vector lengths
 * must be at least the reference's (T_ch^2 + (CM-3) T_ch T + (I-1)(CM-2) T^2, resp.
 * I (T_ch T + (VM-1) T^2), CM/VM = the graph's maximum check/variable degree).
 * Fast path (LDS-resident tables) when T_ch == T_dec <= 16 and all degrees <= 16; otherwise a
 * generic reference-indexing path.  flags: IBL_FLAG_FORCE_GENERIC.
 */
int ibl_ib_create(const ibl_graph* g, int32_t T_ch, int32_t T_dec, int32_t imax,
                  const int32_t* cn_lut, int64_t cn_len, const int32_t* vn_lut, int64_t vn_len,
                  const int32_t* match_cn, int64_t mc_len, const int32_t* match_vn, int64_t mv_len,
                  int32_t match, int32_t max_batch, int32_t flags, ibl_ib** out);
/* 1 = LDS fast path, 0 = generic path */
int ibl_ib_path(const ibl_ib* h);
/*
 * Decode path of an IB decoder on the fast path (no reference counterpart; results are identical):
 *   IBL_PATH_AUTO (default)  the fused on-chip kernel when the code fits (E * 4 bytes of messages
 *                            for 8 codewords plus the largest pass's table quads <= 160 KiB,
 *                            check degrees >= 2; e.g. regular (3,6) N=8000, WLAN), else per-pass.
 *                            Tables sit in quads of 4 and the quads in 64-KiB super-regions of two,
 *                            so an odd quad count rounds up (1 quad: 64 KiB, 3 quads: 128 KiB), plus
 *                            1 KiB of raw image per quad: a code whose largest pass needs 3 quads
 *                            (9-12 tables) is fused up to E = 7,420 edges (E * 4 <= 29,680 B), 4
 *                            quads up to 7,164, 1 or 2 quads (<= 8 tables) up to 24,572 / 24,060;
 *                            the per-pass fast path holds at most 4 quads (16 tables) a pass;
 *   IBL_PATH_PASSES          one launch per check / variable pass, messages in HBM;
 *   IBL_PATH_FUSED           the fused kernel (IBL_EUNSUPPORTED if the code does not fit).
 * ibl_ib_path_in_use reports 1 when decodes run the fused kernel.  With the fused kernel the timing
 * API reports each fused launch as one check-node launch.
 */
int ibl_ib_set_path(ibl_ib* h, int32_t path);
int ibl_ib_path_in_use(const ibl_ib* h, int32_t* fused);
/*
 * Small-batch kernels of the fast path (no reference counterpart; outputs identical to the other
 * kernels).  The per-pass fast kernels give every wave one node x 1024 codewords, so a batch of a few
 * codewords — the reference's DVB-S2 driver decodes msg_at_time = 2 (BER_simulation_OpenCL.py:71) —
 * costs what B = 1024 costs; batches B <= max_b instead run kernels whose wave item is up to 64 nodes
 * of one degree (lane = node) x 8 codewords.  Default max_b = 224 (IBL_SMALL_B in the environment when
 * the decoder is created overrides it); 0 turns them off.  The fused on-chip path, when in use, ignores
 * this.  IBL_EUNSUPPORTED if max_b > 0 and the decoder has no fast path.
 */
int ibl_ib_set_small_batch(ibl_ib* h, int32_t max_b);
int ibl_ib_small_batch(const ibl_ib* h, int32_t* max_b);
/*
 * Degree-2 variable fold of the per-pass fast path (no reference counterpart; outputs and stop iterations
 * are identical with and without it): the message of a degree-2 variable to one of its checks is one
 * table lookup F2(channel, message from the other check), so the check pass that computes that message
 * applies the lookup itself and writes the result into the next check pass's inbox; the variable pass
 * skips the variable.  A variable is folded when in both of its checks its edge is one of the last two
 * inputs (ascending column order) of a check of degree >= 3 — every staircase parity variable of a code
 * whose parity columns come last.  *n_folded = number of folded variables (0: none qualify, a check
 * degree above 8, no fast path, or the fold's table does not fit the check pass's LDS).
 * ibl_ib_set_fold switches the fold off / on (default: on); the small-batch kernels and the fused path
 * never fold.
 */
int ibl_ib_folded(const ibl_ib* h, int32_t* n_folded);
int ibl_ib_set_fold(ibl_ib* h, int32_t on);
/*
 * Composite final step of the per-pass fast path's check chains (no reference counterpart; outputs and stop
 * iterations are identical with and without it): for one check degree D* >= 5 the last two table steps of outputs
 * 0 .. D*-3, "-> L(., x_{D*-2}) -> F(., x_{D*-1})", are composed on the host at create into one table
 * C(t, m)[y] = F(L(t, m), y) of 16 nibbles per entry, and the check pass takes them as one 4-byte LDS read and a
 * nibble select instead of two one-byte reads.  D* is the degree >= 5 with the most checks (ties: the larger);
 * the composite needs the degree <= 8 per-pass kernels and 64 KiB of LDS behind the check pass's tables, which must
 * fit one 64-KiB super-region (up to 8 tables: DVB-S2 with matching has 7).  *degree = D*, or 0: no composite
 * (none planned, or switched off).  ibl_ib_set_composite switches it off / on (default: on); the small-batch
 * kernels, the generic and the fused path never use it.
 */
int ibl_ib_composite(const ibl_ib* h, int32_t* degree);
int ibl_ib_set_composite(ibl_ib* h, int32_t on);
/*
 * The same step for the per-pass variable chains (outputs 0 .. D*-3 of a degree-D* variable end in raw table D*-3
 * and the degree's final table): D* is the variable degree in 5..8 with the most nodes among the variables the pass
 * walks - with the degree-2 fold on, the ones it leaves, whose tables alone are then staged (DVB-S2 with matching:
 * 8, one super-region; with the fold off 9: no composite).  Same LDS rule, same kernels, identical results.
 */
int ibl_ib_vn_composite(const ibl_ib* h, int32_t* degree);
int ibl_ib_set_vn_composite(ibl_ib* h, int32_t on);
/*
 * Codewords per workgroup the fused kernel runs a batch of B with (no reference counterpart; results are
 * identical either way): 8, or 4 (half groups) when 2 * ceil(B / 8) workgroups fit the grid or the
 * environment IBL_FUSED_NCW=4 forces them and the half-group kernel fits the device; 0 when decodes do
 * not run the fused kernel.
 */
int ibl_ib_fused_ncw(const ibl_ib* h, int32_t B, int32_t* ncw);
/*
 * Decode B codewords.  Replaces decode_OpenCL (discrete_LDPC_decoder_irreg.py:245-341;
 * discrete_LDPC_decoder.py:202-295).
 *   d_ch   [N][B] channel cluster ids (IBL_U8 or IBL_I32), values in [0, T_ch)
 *   d_out  [N][B] decided cluster ids (IBL_U8 or IBL_I32); bit = (id < T_dec/2)
 *   early_stop  1: stop when the whole batch has zero syndrome (reference behaviour);
 *               0: run exactly imax iterations (benchmark / decode_on_host behaviour)
 *   d_iters     optional device int32 receiving the iteration index used for the output
 *               (the reference's i_num - 1), NULL to skip
 * Buffers: d_ch and d_out are contiguous and need only their element type's alignment (1 byte for
 * IBL_U8, 4 for IBL_I32) — the kernels take their vector loads and stores only where the pointer and B
 * allow them, and write nothing outside the [N][B] elements of d_out.  d_out may be d_ch itself when
 * both have the same dtype (the channel is staged into the decoder's own buffers before any output is
 * written); buffers that overlap in any other way are not supported.  All work is enqueued on `stream`;
 * a decoder serves one decode at a time (successive decodes of one handle belong on one stream, or are
 * ordered by the caller).
 */
int ibl_ib_decode(ibl_ib* h, const void* d_ch, int32_t ch_dtype, int32_t B, void* d_out, int32_t out_dtype,
                  int32_t early_stop, int32_t* d_iters, void* stream);
void ibl_ib_destroy(ibl_ib* h);
/*
 * Kernel timing for the benchmark (no reference counterpart): when enabled, every check-node and
 * variable-node launch of ibl_ib_decode / ibl_float_decode is bracketed by HIP events on the
 * decode stream.  *_read synchronises those events, returns the summed milliseconds and launch
 * counts since the last read (kernels that exited early through the stop flags included), and
 * clears them.
 */
int ibl_ib_timing(ibl_ib* h, int32_t enable);
int ibl_ib_timing_read(ibl_ib* h, double* cn_ms, int32_t* cn_launches, double* vn_ms, int32_t* vn_launches);

/*
 * Float min-sum / belief-propagation decoder.
 * Replaces Min_Sum_Decoder_class_irregular / BeliefPropagationDecoderClassIrregular
 * .init_OpenCL_decoding (min_sum_decoder_irreg.py:167-218, bp_decoder_irreg.py:167-218).
 * kind = IBL_MINSUM | IBL_BP; precision = IBL_F32 (BASELINE build) | IBL_F64 (the reference's
 * double precision); llr_max = clamp of BP / VN messages (the reference's LLR_MAX = 150).
 * Degrees (ibl_float_create and ibl_float_create_corrected alike): check degrees up to 32, variable degrees up to
 * 16; a code outside either range is IBL_EUNSUPPORTED, and ibl_last_error names the kind of node, the limit and the
 * code's largest degree of that kind.  A handle whose code has a check of degree above 16 is WIDE
 * (ibl_float_is_wide; DVB-S2 normal frames at rates 4/5 to 9/10, 5G NR base graph 1): its check passes and its fused
 * kernel are instantiations of their own, in which checks of degree 17..32 run one body that takes the degree at
 * run time, and checks of degree 2..16 the bodies of a narrow handle.  A narrow handle runs exactly the kernels it
 * ran before wide handles existed.  The semantics are the same at every degree: min-sum magnitudes are the minimum
 * over the other inputs, signs the XOR of their signs, bit-identical to the reference's fold; corrected min-sum
 * applies its two rounded operations to the (minimum, second minimum) pair; fp64 BP folds the other inputs in the
 * reference's order for every output; fp32 BP keeps its forward-backward association order, extended to the
 * degree.  The three kernel families (per pass, small batch, fused) give the same bits, the per-pass path folds
 * degree-2 variables, and the per-codeword stop runs on a wide handle that takes the fused kernel, as on a narrow one.
 */
int ibl_float_create(const ibl_graph* g, int32_t kind, int32_t imax, double llr_max, int32_t precision,
                     int32_t max_batch, ibl_float** out);
/*
 * Replaces decode_OpenCL_min_sum (min_sum_decoder_irreg.py:221-287) and
 * decode_OpenCL_belief_propagation (bp_decoder_irreg.py:221-286).
 *   d_llr [N][B] channel LLRs (IBL_F32 / IBL_F64), d_out [N][B] APP LLRs (IBL_F32 / IBL_F64)
 * Precondition: no channel LLR is NaN.  Min-sum allows +-inf (a known bit: every message a variable
 * sends is clamped to +-llr_max, its APP LLR is +-inf), and every message stays finite.  BP box-pluses raw
 * channel values in the first check pass (later box-plus inputs are clamped to +-llr_max): the fp64 decoder
 * (the reference's formula log((1 + e^(a+b)) / (e^a + e^b)), kernels_min_and_BP.cl:5-9) needs
 * |x| <= 709.089, just under ln(DBL_MAX / 2) = 709.0895657... — beyond that, two same-sign values overflow the
 * denominator beside an infinite numerator and the reference gives NaN (inf / inf); within it an overflowing
 * numerator or vanishing denominator gives +-inf, clamped to +-llr_max as in the reference — and the fp32
 * decoder (an overflow-free form of the same function) needs finite values.  The float kernels take min /
 * max / median as single instructions that assume non-NaN operands: a NaN input gives unspecified outputs.
 * Dtypes: llr_dtype and out_dtype are independent of the decoder's precision.  A channel LLR of the other
 * dtype is converted to the decoder's precision once, when it is staged: IBL_F32 -> fp64 exactly,
 * IBL_F64 -> fp32 by round-to-nearest-even (a finite value beyond FLT_MAX becomes +-inf, and it is the
 * staged value the precondition above applies to for the fp32 decoder); the decode is then the one of
 * those staged values.  An APP LLR is converted from the decoder's precision to out_dtype the same way
 * (fp32 -> IBL_F64 exactly, fp64 -> IBL_F32 by round-to-nearest-even).
 * Buffers: d_llr and d_out are contiguous and need only their element type's alignment (4 bytes for
 * IBL_F32, 8 for IBL_F64) — vector loads and stores are taken only where the pointer and B allow them, and
 * nothing outside the [N][B] elements of d_out is written.  d_out may be d_llr itself when both have the
 * same dtype (the channel is staged into the decoder's own buffers before any output is written); buffers
 * that overlap in any other way are not supported.  All work is enqueued on `stream`; a decoder serves one
 * decode at a time.
 */
int ibl_float_decode(ibl_float* h, const void* d_llr, int32_t llr_dtype, int32_t B, void* d_out,
                     int32_t out_dtype, int32_t early_stop, int32_t* d_iters, void* stream);
void ibl_float_destroy(ibl_float* h);
/*
 * Decode path of a float decoder (no reference counterpart; results are identical on both):
 *   IBL_PATH_AUTO (default)  the fused on-chip kernel when the code fits in LDS ((E + N) * 16 bytes of
 *                            messages and channel plus 2 bytes per variable edge slot index — each
 *                            variable task's rows padded to 64 — within 160 KiB, E < 65536, check
 *                            degrees >= 2), else IBL_PATH_PASSES;
 *   IBL_PATH_PASSES          one launch per check / variable pass, messages in HBM;
 *   IBL_PATH_FUSED           the fused kernel (IBL_EUNSUPPORTED if the code does not fit).
 * ibl_float_path_in_use reports 1 when decodes run the fused kernel, 0 otherwise.  With the fused
 * kernel the timing API reports each fused launch as one check-node launch (vn counts stay 0).
 */
int ibl_float_set_path(ibl_float* h, int32_t path);
int ibl_float_path_in_use(const ibl_float* h, int32_t* fused);
/*
 * Launch geometry of the fused kernel for a batch of B (no reference counterpart; read-only, the values
 * ibl_float_decode uses): *ngroups = groups of 4 fp32 / 2 fp64 codewords, ceil(B / 4) or ceil(B / 2);
 * *grid = workgroups launched, min(ngroups, blocks per CU x CUs) — workgroup w decodes groups w, w + grid,
 * w + 2 grid, ...  Both 0 when decodes do not run the fused kernel.
 */
int ibl_float_fused_geometry(const ibl_float* h, int32_t B, int32_t* ngroups, int32_t* grid);
/*
 * Degree-2 variable fold of the per-pass path (no reference counterpart; outputs are identical with and
 * without it): the check pass that produces a degree-2 variable's input also computes that variable's
 * output message (clamp(ch + m), kernels_min_and_BP.cl:110-118) into the next check pass's inbox, and the
 * variable pass skips the variable.  *n_folded = number of folded variables (0: off — no degree-2
 * variables, or IBL_FL_FOLD=0 in the environment when the decoder was created).
 */
int ibl_float_folded(const ibl_float* h, int32_t* n_folded);
/*
 * *wide = 1 for a handle whose code has a check of degree above 16 (see ibl_float_create), else 0.  Read-only; as
 * ibl_layered_is_wide for the layered decoders.
 */
int ibl_float_is_wide(const ibl_float* h, int32_t* wide);
/*
 * Small-batch kernels of the per-pass float path (no reference counterpart; outputs identical): batches
 * B <= max_b run kernels whose wave item is up to 64 nodes of one degree (lane = node) x 4 fp32 / 2 fp64
 * codewords instead of one node x 256 / 128 codewords; they do not fold.  Default max_b = 64
 * (IBL_SMALL_B at create overrides it); 0 turns them off.  The fused path, when in use, ignores this.
 */
int ibl_float_set_small_batch(ibl_float* h, int32_t max_b);
int ibl_float_small_batch(const ibl_float* h, int32_t* max_b);
/*
 * Channel-LLR precondition check (no reference counterpart).  The staging step of every ibl_float_decode
 * counts the channel LLRs that break ibl_float_decode's precondition — NaN (min-sum); NaN or |x| > 709.089
 * (BP, fp64 decoder); NaN or +-inf (BP, fp32 decoder) — on the device, without a host sync, into one counter
 * per decoder.  This call synchronises the decoder's DEVICE (every stream: the count covers all decodes of
 * this decoder enqueued since the previous call, whatever their stream; `stream` is unused), stores that
 * count in *violations (may be NULL), clears it, and returns IBL_EINVAL (message in ibl_last_error) when it
 * is not 0: the outputs of those decodes are unspecified.  A caller that wants the verdict of one decode
 * calls it once before that decode (to clear) and once after (the reference-named classes do so for every
 * decode that returns host arrays).
 */
int ibl_float_input_check(ibl_float* h, int32_t* violations, void* stream);
int ibl_float_timing(ibl_float* h, int32_t enable);
int ibl_float_timing_read(ibl_float* h, double* cn_ms, int32_t* cn_launches, double* vn_ms, int32_t* vn_launches);
/*
 * Corrected min-sum: normalised / offset min-sum on the flooding float decoder (no reference counterpart: the
 * reference's min-sum is uncorrected).  A third arithmetic of ibl_float beside plain min-sum and BP, fixed when
 * the decoder is created.  Let F be the decoder's precision (fp32 or fp64), a = (F)alpha and b = (F)beta, each
 * converted once from the double arguments by round-to-nearest-even.  For check c and output edge w, over the
 * inputs m_j of the other edges:
 *   M   = min over j != w of |m_j|
 *   s   = XOR over j != w of (m_j < 0)
 *   t   = a * M          one rounded multiplication in F
 *   u   = t - b          one rounded subtraction in F   (no fused multiply-add)
 *   r   = max(u, 0)
 *   out = s ? -r : r
 * The sign of a zero result is not specified: a zero magnitude makes every sign that depends on it immaterial to
 * any later value (sums take it as 0, minima as magnitude 0, and the syndrome is taken on < 0), and all
 * comparisons are by value.  This closed form is the definition; the underflow caveat of plain min-sum's fold
 * does not apply.  Everything else is the min-sum decoder above, operation for operation: the first send is the
 * raw channel value; the variable update adds the channel first, then the ascending edges, and is clamped to
 * +-llr_max; the APP output is unclamped; the syndrome is taken on < 0 of the variable-to-check messages;
 * imax - 1 iterations run; the early stop is batch-global and d_iters is one word; the NaN precondition and
 * +-inf channel values are handled as for min-sum (ibl_float_decode, ibl_float_input_check).
 * Parameter domain: alpha finite with 0 < alpha <= 1, beta finite with beta >= 0, and the same of the converted
 * values a and b (an alpha that rounds to 0 or a beta that rounds to infinity in an fp32 decoder is refused; beta =
 * -0.0 is taken, and reported, as +0); anything else is IBL_EINVAL, reported (like imax, max_batch and precision
 * errors) before a NULL graph is.  (1, 0) is plain min-sum: it
 * creates the decoder ibl_float_create(IBL_MINSUM) creates, with the same kernels.  The handle is an ibl_float in
 * every other respect (decode, paths, small batches, fold, input check, timing); two decoders with different
 * corrections may coexist on one device.
 * ibl_float_correction reports the pair: (1, 0) on plain min-sum handles, IBL_EINVAL on BP handles.
 */
int ibl_float_create_corrected(const ibl_graph* g, double alpha, double beta, int32_t imax, double llr_max,
                               int32_t precision, int32_t max_batch, ibl_float** out);
int ibl_float_correction(const ibl_float* h, double* alpha, double* beta);
/*
 * Per-codeword stop on the fused flooding decoders (no reference counterpart: the reference stops a batch when every
 * codeword's syndrome is zero).  ibl_ib_decode_each and ibl_float_decode_each take the arguments of ibl_ib_decode /
 * ibl_float_decode without early_stop; d_iters is NULL or B int32 entries.
 * For codeword c of a batch, d_out[:, c] and d_iters[c] are exactly what today's decoder produces when it decodes
 * column c alone (B = 1) with early_stop = 1, and d_iters[c] = L_c:
 *   IB     L_c is the first check pass j >= 1 whose inputs have a zero syndrome for c, else imax - 1; the output is
 *          the decision with the decision tables of pass L_c on the messages check pass L_c wrote;
 *   float  L_c is the first iteration i >= 1 whose variable-to-check messages have a zero syndrome for c (the
 *          syndrome check pass i + 1 reads), else imax - 1; the output is the APP LLRs of iteration L_c (channel
 *          plus all check-to-variable messages of check pass L_c).
 * The result of a codeword does not depend on its neighbours, on the group size (IB 8 or 4 codewords a workgroup,
 * float 4 fp32 / 2 fp64), on the grid or on the number of CUs.  With imax == 1 it equals the fixed-iteration
 * decode and d_iters[c] = 0.  Codewords that share a group keep iterating until the whole group has stopped; a
 * codeword that stopped earlier keeps the output of its own L_c, and whatever happens to its messages afterwards
 * reaches neither d_out nor d_iters.  Columns past the end of the batch are never running and never written, and
 * nothing outside the [N][B] elements of d_out and the B entries of d_iters is written.
 * One staging launch and one kernel launch per decode: no flag words, no second pass.  Both run on the fused kernel
 * only and return IBL_EUNSUPPORTED, launching nothing, when the handle's decodes would not run it (IBL_PATH_PASSES,
 * a code that does not fit, the generic IB path; ibl_ib_path_in_use / ibl_float_path_in_use).  The float entry
 * takes all three arithmetics (min-sum, corrected min-sum, BP) in both precisions; both take every channel / output
 * dtype of their decode; d_out may be d_llr as in ibl_float_decode, `stream` as there, and the float staging
 * counts precondition violations as there (ibl_float_input_check).
 */
int ibl_ib_decode_each(ibl_ib* h, const void* d_ch, int32_t ch_dtype, int32_t B, void* d_out, int32_t out_dtype,
                       int32_t* d_iters, void* stream);
int ibl_float_decode_each(ibl_float* h, const void* d_llr, int32_t llr_dtype, int32_t B, void* d_out,
                          int32_t out_dtype, int32_t* d_iters, void* stream);

/*
 * Layered min-sum: layered (row-serial) normalised / offset min-sum decoding, fp32 (no reference counterpart:
 * the reference's decoders are flooding decoders with uncorrected min-sum).
 *
 * Layers: an ordered list of disjoint sets of checks that together cover all checks; within one layer no
 * variable appears in two checks.  layer_ptr[n_layers + 1] (layer_ptr[0] = 0) delimits the layers in
 * layer_checks[n_c].  For a quasi-cyclic code the block rows are layers.  (codes.dvbs2_layers: in a DVB-S2 code
 * the q = (n - k) / 360 residue classes {r, r + q, r + 2q, ...} of the checks are valid layers — bit m of an
 * information group meets check (x + m q) mod (n - k), one check of a class per address as long as a group has no
 * two addresses of one residue, and a staircase parity variable joins checks j and j + 1, never two of a class.)
 *
 * Semantics, per codeword; every operation is one individually rounded fp32 operation (no FMA):
 *   P[v] = channel LLR;  R[e] = 0 for every edge
 *   for it = 1..imax:
 *     for each layer in order, for each check c of the layer (any order):
 *       for the edges e = (c, v) of c in ascending column order:
 *           Q_e = clamp(P[v] - R[e], -llr_max, +llr_max);  neg_e = (Q_e < 0)
 *       m1 = min |Q_e|, at the FIRST position attaining it;  m2 = min over the other positions;  s = XOR neg_e
 *       for each e:  mag = (e is that first position) ? m2 : m1
 *                    mag = max(alpha * mag - beta, 0)      (the product rounded, then the difference rounded)
 *                    R[e] = (s ^ neg_e) ? -mag : mag;   P[v] = Q_e + R[e]
 *     if early_stop: x = (P < 0); a codeword whose syndrome H x is zero for the first time now has
 *                    out[:, b] = P[:, b], iters[b] = it, and is finished
 *   codewords never finished: out[:, b] = P after imax iterations, iters[b] = imax
 *   early_stop = 0: no syndrome, every codeword runs imax iterations, iters[b] = imax
 * alpha = 1, beta = 0 is plain layered min-sum.  The early stop is PER CODEWORD (the flooding decoders above
 * stop the whole batch together, as the reference does).
 * Preconditions: channel LLRs finite; check degrees in [2, 32] (else IBL_EUNSUPPORTED).
 *
 * Narrow and wide handles.  A handle is WIDE when its code has a check of degree above 16 (DVB-S2 normal frames of
 *   rates 4/5 .. 9/10: degrees 18, 22, 27, 30; 5G NR base graph 1: 19); every other handle is narrow, and for it
 *   every statement below holds as written.  A wide handle keeps, for EVERY check of its code, the sign bits of R
 *   in a whole 32-bit word and the argmin position in a word of its own — four 4-byte words per check and codeword
 *   (corrected m1, corrected m2, sign bits, position) where a narrow handle keeps three — and runs kernels of its
 *   own for the steps that touch that state (the fused kernel, the staging launch, the layer launches and the row
 *   move of the compaction).  Read for a wide handle:  12 n_c -> 16 n_c  in the fit rule
 *   cw_per_group = min(8, floor(160 KiB / (4 N + 16 n_c))) (IBL_PATH_AUTO judges a wide code by it, and the "does
 *   not fit" message names it) and in the per-layer memory (about 4 N + 16 n_c bytes per codeword of max_batch: a
 *   fourth [n_c][ldb] array; an iteration moves 8 E + 32 n_c bytes per codeword);  n_v + 3 n_c -> n_v + 4 n_c  rows
 *   in the compaction's row move.  The semantics, the launch chain and its count per decode, the stop masks, the
 *   packed hard decisions, the syndrome and finalise kernels and the "no allocation, no host synchronisation,
 *   capturable" guarantee are the same.  ibl_layered_is_wide tells which kind a handle is.
 *
 * ibl_layers_validate  (host only, no device) checks cover, disjointness, no variable shared within a layer
 *   (IBL_EINVAL) and the degree range (IBL_EUNSUPPORTED); ibl_last_error names the first offending check.
 * ibl_layered_create   validates the layers, builds the device plan and allocates a [max_batch][N] fp32 staging
 *   buffer.  alpha, beta >= 0, llr_max > 0 (the project's value: 150).  precision: IBL_F32; IBL_F64 returns
 *   IBL_EUNSUPPORTED (fp64 is not built; layered BP is ibl_layered_create_bp, "Layered BP" below).
 *   Fit rule: the decoder is one fused on-chip kernel — one wave owns one codeword, whose APP LLRs (4 N bytes)
 *   and compressed check state (12 bytes per check: corrected m1, m2, argmin position | sign bits) stay in LDS
 *   through all iterations.  A workgroup holds cw_per_group = min(8, floor(160 KiB / (4 N + 12 n_c))) codewords;
 *   IBL_EUNSUPPORTED when that is 0 (N = 1944 rate 1/2: 19,440 B, 8 codewords; DVB-S2 N = 64800: 648 KB, does
 *   not fit).  It is ibl_layered_create_path with IBL_PATH_FUSED.
 * ibl_layered_create_path  the same with a choice of kernels:
 *     IBL_PATH_FUSED   the fused on-chip kernel above (IBL_EUNSUPPORTED when the code does not fit);
 *     IBL_PATH_PASSES  per-layer kernels over HBM for codes of any length that pass ibl_layers_validate (codes
 *                      that would fit the fused kernel included): lane = codeword, one launch per layer, a wave
 *                      updating one check for 64 codewords;
 *     IBL_PATH_AUTO    the fused kernel when the code fits, else the per-layer kernels;
 *   any other value is IBL_EINVAL; IBL_F64 is IBL_EUNSUPPORTED on every path.  The semantics are those specified
 *   above on every path, the per-codeword stop included: a finished codeword's APP values are frozen at its stop
 *   iteration.  A per-layer handle owns, allocated at create for max_batch rounded up to 64 codewords, the APP
 *   LLRs [N][ldb] fp32 and the compressed state of every check (3 x [n_c][ldb] 4-byte words: corrected m1, m2,
 *   argmin position | sign bits), the packed hard decisions (one bit per variable and codeword), one 64-bit mask
 *   of finished and one of unsatisfied codewords per 64 codewords and one counter of running codewords: about
 *   (4 N + 12 n_c) bytes per codeword of max_batch (DVB-S2 N = 64800 rate 1/2 at 8192 codewords: 5.3 GB).
 *   ibl_layered_decode on such a handle enqueues one staging launch, n_layers launches per iteration, three more
 *   (pack the hard decisions, syndrome, finalise) after every iteration but the last when early_stop is set, and
 *   one output launch, all on `stream`: no allocation, no host synchronisation and no host read-back, so a
 *   caller may capture it.  Finished codewords are skipped per whole tile of 64.  IBL_LAY_SYNDROME=gather in the
 *   environment at create selects the syndrome's other form (one launch that gathers the sign bits per check;
 *   same results, measured slower: DESIGN.md); any value but gather / packed is IBL_EINVAL.
 * ibl_layered_path_in_use  *fused = 1 when decodes run the fused kernel, 0 for the per-layer kernels.
 * ibl_layered_is_wide  *wide = 1 for a handle (fp32 or fixed point) whose code has a check of degree above 16, else
 *   0; NULL arguments are IBL_EINVAL.
 * ibl_layered_decode  d_llr [N][B] IBL_F32 in, d_out [N][B] IBL_F32 APP LLRs out, d_iters [B] int32 (or NULL):
 *   iterations run per codeword.  Asynchronous on `stream`, no host synchronisation.
 * ibl_layered_geometry the launch geometry ibl_layered_decode uses for a batch of B: codewords per workgroup,
 *   *ngroups = ceil(B / cw_per_group) groups of consecutive codewords, *grid = workgroups launched,
 *   min(ngroups, blocks per CU x CUs) — workgroup w decodes groups w, w + grid, w + 2 grid, ...  All three
 *   are 0 on a per-layer handle (the convention of ibl_float_fused_geometry).
 *
 * Compaction of the running codewords (fp32 per-layer handles; off unless switched on).  The per-layer kernels
 *   skip finished codewords per whole tile of 64 only, so near the waterfall a few running codewords scattered over
 *   the batch keep most tiles alive.  With compaction on, after the stop check of every iteration `it` with
 *   it % every == 0 the device moves the columns of the running codewords to the lowest columns of P and of the
 *   check state, in their order, and writes the finished codewords it drops to d_out at that moment.  Policy, with
 *   R running codewords in an extent of E columns (E = B at the start), tE = ceil(E / 64), tR = ceil(R / 64):
 *       compact  iff  R > 0  and  tE - tR >= max(1, ceil(min_free_pct * tE / 100));   afterwards E = R.
 *   The decision is taken on the device: ibl_layered_decode still enqueues every launch up front (three more per
 *   attempt: plan, row move, commit; the last two leave at once when the plan declined), allocates nothing and reads
 *   nothing back, and no kernel waits for another workgroup.  Every value of d_out and d_iters is what the decode
 *   without compaction gives, bit for bit.  d_out may be written before the decode's last kernel, and d_out may
 *   still be d_llr: d_llr is read by the first launch only.
 * ibl_layered_set_compaction  every = 0 switches it off (min_free_pct is not looked at); every >= 1 with
 *   1 <= min_free_pct <= 100 switches it on for the decodes that follow, allocating on first use 8 bytes per
 *   codeword of max_batch rounded up to 64, and 16 more.  Other numbers, judged first, and h == NULL are
 *   IBL_EINVAL; a handle of the fused kernel is IBL_EUNSUPPORTED ("compaction needs the per-layer path"), a
 *   fixed-point handle too ("compaction is not built for the fixed-point decoder").
 * ibl_layered_compaction_stats  a diagnostic read-back: waits for `stream` (the stream of the last decode; no other
 *   stream is waited for) and gives the compactions that decode made and its final extent; 0 and B after a decode
 *   without compaction.  Refusals as ibl_layered_set_compaction.
 */
typedef struct ibl_layered ibl_layered;
int ibl_layers_validate(int32_t n_v, int32_t n_c, const int32_t* csr_indptr, const int32_t* csr_cols,
                        int32_t n_layers, const int32_t* layer_ptr, const int32_t* layer_checks);
int ibl_layered_create(const ibl_graph* g, int32_t n_layers, const int32_t* layer_ptr, const int32_t* layer_checks,
                       int32_t imax, float alpha, float beta, float llr_max, int32_t precision, int32_t max_batch,
                       ibl_layered** out);
int ibl_layered_create_path(const ibl_graph* g, int32_t n_layers, const int32_t* layer_ptr,
                            const int32_t* layer_checks, int32_t imax, float alpha, float beta, float llr_max,
                            int32_t precision, int32_t max_batch, int32_t path, ibl_layered** out);
int ibl_layered_path_in_use(const ibl_layered* h, int32_t* fused);
int ibl_layered_is_wide(const ibl_layered* h, int32_t* wide);
int ibl_layered_decode(ibl_layered* h, const void* d_llr, int32_t llr_dtype, int32_t B, void* d_out,
                       int32_t out_dtype, int32_t early_stop, int32_t* d_iters, void* stream);
int ibl_layered_geometry(const ibl_layered* h, int32_t B, int32_t* cw_per_group, int32_t* ngroups, int32_t* grid);
int ibl_layered_set_compaction(ibl_layered* h, int32_t every, int32_t min_free_pct);
int ibl_layered_compaction_stats(const ibl_layered* h, void* stream, int32_t* compactions, int32_t* extent);
void ibl_layered_destroy(ibl_layered* h);

/*
 * Layered BP: layered (row-serial) belief propagation, fp32.  Layers, the per-codeword early stop, iters[] and out[]
 * are those of "Layered min-sum" above; the check update is the box-plus of the flooding fp32 BP decoder.
 *
 * Semantics, per codeword:
 *   P[v] = channel LLR;  R[e] = 0
 *   for it = 1..imax:
 *     for each layer in order, each check c of it, edges e_0..e_{D-1} in ascending column order:
 *         Q_k = P[v_k] - R[e_k]                        (one rounded subtraction, NOT clamped)
 *         D == 2:  R'_0 = clamp(Q_1), R'_1 = clamp(Q_0)
 *         D >= 3:  S_{D-1} = Q_{D-1};  S_j = Q_j [+] S_{j+1}  (j = D-2 .. 1)
 *                  R'_0 = S_1;  F = Q_0
 *                  for w = 1 .. D-2:  R'_w = F [+] S_{w+1};  F = Q_w [+] F
 *                  R'_{D-1} = F                          (3(D-2) box-pluses)
 *         R[e_k] = R'_k;   P[v_k] = Q_k + R'_k          (one rounded addition)
 *     early stop, iters[], out[]: exactly as "Layered min-sum" (per codeword, frozen at the stop)
 *   a [+] b is the fp32 box-plus of the flooding BP check node: magnitude
 *     min(|a|,|b|) + ln(1 + e^-(|a|+|b|)) - ln(1 + e^-||a|-|b||) on the hardware's base-2 exp / log, clamped to
 *     [0, llr_max], sign sgn(a) sgn(b).  It clamps its result, so S_j, F and every R' of a check of degree >= 3 lie
 *     in [-llr_max, llr_max]; clamp is the clamp to +-llr_max, needed for the degree-2 messages only.
 *   Why Q is not clamped (the layered min-sum rule, Q = clamp(P - R), P = Q + R, is unstable with box-plus messages):
 *     once that clamp bites, P loses the other checks' contributions, and the next check sees a small Q for a
 *     variable that was firmly known.  WLAN N = 648 at 2.5 dB with llr_max 30 then leaves NO codeword of 64 with a
 *     zero syndrome from iteration 10 on; with the rule above all 64 stay converged (tests/test_cpu_layered_bp.py).
 *     |P| is bounded by |llr| + (variable degree) * llr_max.
 *   Preconditions: channel LLRs finite, |llr| + 16 * llr_max below FLT_MAX.
 *   Supported: check degrees 2..16 (a check above 16 is IBL_EUNSUPPORTED, the message names it), variable degrees
 *   up to 16 (what the precondition's bound covers; no kernel depends on the variable degree), IBL_F32 only.
 *   Parity with this specification is by value (|x - y| <= 1e-5 max(|x|, |y|) + 1e-4 against an fp64 evaluation), not
 *   bit for bit: the transcendentals are the hardware's.  The two paths below run one check core in one operation
 *   order and give each other's bits.
 *
 * ibl_layered_create_bp  validates as ibl_layered_create_path (llr_max > 0 and finite).  IBL_F64 is IBL_EUNSUPPORTED
 *   ("fp64 is not built").  path:
 *     IBL_PATH_FUSED   one wave owns one codeword: P[N] and R[E], one fp32 word per edge, stay in LDS through all
 *                      iterations (lane = check; the task walk, stop, group loop and transposed staging of the
 *                      min-sum fused kernel).  Fit rule: cw_per_group = min(8, floor(160 KiB / (4 N + 4 E)));
 *                      IBL_EUNSUPPORTED when that is 0 (N = 1944 rate 1/2, E = 6,966: 35,640 B, 4 codewords; DVB-S2
 *                      N = 64800 does not fit).  R is laid out task by task, edge k of lane i of a task of `count`
 *                      checks at rfirst + count k + i: the lanes touch consecutive words, and R is exactly E words.
 *     IBL_PATH_PASSES  per-layer kernels over HBM: P [N][ldb] and R [E][ldb] fp32 (a row per edge), lane = codeword,
 *                      one launch per layer, a wave updating one check for 64 codewords.  The masks, the packed
 *                      syndrome, finalise and output launches are the min-sum path's.  The first iteration takes
 *                      R = 0 without reading or zeroing the E rows.  An iteration moves 16 E bytes per codeword
 *                      (P and R of every edge read and written), the first 12 E.  The handle owns about 4 N + 4 E
 *                      bytes per codeword of max_batch rounded up to 64: DVB-S2 N = 64800 rate 1/2 (E = 226,799)
 *                      1.17 MB per codeword, 9.6 GB at 8192.  Launch chain, "no allocation, no host
 *                      synchronisation, capturable" as on the min-sum per-layer path.
 *     IBL_PATH_AUTO    the fused kernel when the code fits by the rule above, else the per-layer kernels.
 *   The handle is an ibl_layered: ibl_layered_decode (IBL_F32 in and out), _path_in_use, _geometry and _destroy work
 *   as documented above; ibl_layered_is_wide and ibl_layered_is_fixed give 0; ibl_layered_set_compaction and
 *   ibl_layered_compaction_stats return IBL_EUNSUPPORTED ("compaction is not built for the BP decoder").
 * ibl_layered_is_bp  *bp = 1 for a handle of ibl_layered_create_bp, else 0; NULL arguments are IBL_EINVAL.
 */
int ibl_layered_create_bp(const ibl_graph* g, int32_t n_layers, const int32_t* layer_ptr, const int32_t* layer_checks,
                          int32_t imax, float llr_max, int32_t precision, int32_t max_batch, int32_t path,
                          ibl_layered** out);
int ibl_layered_is_bp(const ibl_layered* h, int32_t* bp);

/*
 * Layered BP, half-precision state: the "Layered BP" decoder above with its two state arrays, P and R, stored as IEEE
 * binary16 and every operation still done in fp32.  It halves the bytes an iteration moves on the per-layer path and
 * the LDS a codeword takes in the fused kernel.  Layers, the per-codeword early stop, iters[] and out[] are those of
 * "Layered BP".
 *
 *   h(x) = round-to-nearest-even to binary16 of clamp(x, -65504, +65504)   (subnormal halves are kept)
 *   f(y) = the exact conversion of a binary16 value to fp32
 *
 * Semantics, per codeword:
 *   P[v] = h(llr[v] + 0);  R[e] = +0
 *   for it = 1..imax:
 *     for each layer in order, each check c of it, edges e_0..e_{D-1} in ascending column order:
 *         Q_k    = f(P[v_k]) - f(R[e_k])               (one rounded fp32 subtraction, NOT clamped)
 *         R'_k   : the fp32 forward-backward box-plus order of "Layered BP" on the Q_k
 *                  (D == 2: R'_0 = clamp(Q_1), R'_1 = clamp(Q_0), the clamp to +-llr_max)
 *         R[e_k] = h(R'_k)
 *         P[v_k] = h(Q_k + f(R[e_k]))                   (one rounded fp32 addition, with the ROUNDED message)
 *     early stop: as "Layered BP", on the decisions x_v = (f(P[v]) < 0) BY VALUE: h turns a tiny negative sum into
 *       -0, which decides 0 (the fp32 decoders never hold a -0; no kernel of this decoder reads a sign bit)
 *   out[v][b] = f(P[v]) of codeword b, frozen at its stop; iters[] as "Layered BP".
 *   Every output value is therefore a binary16 value.
 *   The result is defined for every finite input: the clamp in h precedes the conversion, so nothing becomes inf or
 *   NaN.  The bound |P| <= |llr| + d_v * llr_max of "Layered BP" holds only while |llr| + 16 * llr_max <= 65504;
 *   beyond that P saturates at +-65504, the sums above lose the other checks' contributions and the decoder no
 *   longer decodes meaningfully.  Precondition for meaningful decoding: channel LLRs finite and
 *   |llr| + 16 * llr_max <= 65504 (llr_max = 150: |llr| <= 63,104).
 *   Input and output stay [N][B] IBL_F32; binary16 input and output are not built.
 *   Supported: check degrees 2..16 (a check of degree 17 or more is IBL_EUNSUPPORTED, the message names it), variable
 *   degrees up to 16.
 *   Parity with this specification is by value, not bit for bit, wherever a box-plus is evaluated: the
 *   transcendentals are the hardware's.  (A code whose checks all have degree 2 has no box-plus and is decoded bit
 *   for bit.)  The two paths below run one check core in one operation order and give each other's bits.
 *
 * ibl_layered_create_bp_half  validates as ibl_layered_create_bp, in its order and with its messages (there is no
 *   precision argument).  path:
 *     IBL_PATH_FUSED   the fused kernel of "Layered BP" with the wave's LDS slice P16[N] | R16[E].  Fit rule:
 *                      cw_bytes = 2 N + 2 E rounded up to 4, cw_per_group = min(8, floor(160 KiB / cw_bytes));
 *                      IBL_EUNSUPPORTED when that is 0, the message naming "2 N + 2 E" (N = 1944 rate 1/2:
 *                      17,820 B, 8 codewords a workgroup where the fp32 state holds 4; DVB-S2 N = 64800 does not
 *                      fit).  The staging is the fp32 kernel's [B][N] fp32 transpose; the wave converts as it reads
 *                      and writes its row.
 *     IBL_PATH_PASSES  per-layer kernels over HBM: P16 [N][ldb] and R16 [E][ldb], a lane owning two consecutive
 *                      codewords (one dword of a row), a wave updating one check for 128 codewords; ldb is max_batch
 *                      rounded up to 128.  The masks of finished and unsatisfied codewords and the packed hard
 *                      decisions stay per 64 codewords (mask words past the batch are all ones), the packed syndrome
 *                      and the finalise launch are the min-sum path's, the pack of the hard decisions and the output
 *                      launch are this decoder's.  The first iteration takes R = 0 without reading or zeroing the E
 *                      rows.  An iteration moves 8 E bytes per codeword, the first 6 E.  The handle owns about
 *                      2 N + 2 E bytes per codeword: DVB-S2 N = 64800 rate 1/2 583 KB per codeword, 4.8 GB at 8192.
 *                      "No allocation, no host synchronisation, no read-back, capturable" as on every per-layer path.
 *     IBL_PATH_AUTO    the fused kernel when the code fits by the rule above, else the per-layer kernels.
 *   The handle is an ibl_layered: ibl_layered_decode (IBL_F32 in and out), _path_in_use, _geometry and _destroy work
 *   as documented above; ibl_layered_is_bp gives 1, ibl_layered_is_wide and ibl_layered_is_fixed give 0;
 *   ibl_layered_set_compaction and ibl_layered_compaction_stats return IBL_EUNSUPPORTED ("compaction is not built for
 *   the BP decoder").
 * ibl_layered_is_half  *half = 1 for a handle of ibl_layered_create_bp_half, 0 for every other handle; NULL arguments
 *   are IBL_EINVAL.
 */
int ibl_layered_create_bp_half(const ibl_graph* g, int32_t n_layers, const int32_t* layer_ptr,
                               const int32_t* layer_checks, int32_t imax, float llr_max, int32_t max_batch,
                               int32_t path, ibl_layered** out);
int ibl_layered_is_half(const ibl_layered* h, int32_t* half);

/*
 * Layered min-sum, fixed point: a second arithmetic of the layered decoder above, integer throughout — 8-bit APP
 * values, messages saturated at q_max (6 bits at most) — on the per-layer path over HBM (ibl_layered_create_fixed) or fused
 * on chip for the codes that fit (ibl_layered_create_fixed_fused).  Layers, the per-codeword
 * early stop, the handle type and ibl_layered_decode / _path_in_use / _geometry / _destroy are those above.
 *
 * Parameters:  alpha16  int 0..16   normalisation in sixteenths (13 is the project's 0.8125)
 *              beta_q   int 0..63   offset in integer units
 *              q_max    int 1..63   message saturation (31: 6-bit messages)
 *              scale    float, finite, > 0   integer units per LLR unit (2.0)
 * The APP saturation is fixed at 127.
 *
 * Semantics, per codeword; all arithmetic in integers:
 *   P[v] = clamp(rint(f32(llr[v]) * f32(scale)), -127, +127)
 *           one rounded fp32 product, rint ties-to-even, clamped as a float before conversion
 *           IBL_I8 input: P[v] = max(x, -127)
 *   R[e] = 0
 *   for it = 1..imax:
 *     for each layer in order, each check c of the layer, its edges e = (c, v) in ascending column order:
 *         T_e = P[v] - R[e]                        (not clamped)
 *         Q_e = clamp(T_e, -q_max, +q_max);  neg_e = (T_e < 0)
 *       m1 = min |Q_e| at the FIRST position attaining it;  m2 = min over the other positions;  s = XOR neg_e
 *       for each e:  mag = (e is that first position) ? m2 : m1
 *                    mag = max(((alpha16 * mag + 8) >> 4) - beta_q, 0)
 *                    R[e] = (s ^ neg_e) ? -mag : mag
 *                    P[v] = clamp(T_e + R[e], -127, +127)
 *     early stop, per codeword: as the fp32 decoder (x = P < 0; the first zero syndrome freezes out and iters)
 *   out:  IBL_I8 -> P;   IBL_F32 -> f32(P) / f32(scale)   (one correctly rounded fp32 division)
 * Precondition: no channel LLR is NaN.  P is updated from the unclamped T, not from Q as in the fp32 semantics:
 * the usual hardware form, which keeps the 8-bit APP range useful when q_max is small.
 *
 * ibl_layered_create_fixed  validates as ibl_layered_create_path does.  Out-of-range parameters, imax or max_batch
 *   < 1 and an unknown path are IBL_EINVAL; IBL_PATH_FUSED is IBL_EUNSUPPORTED (the fixed-point fused kernel is not
 *   built); IBL_PATH_PASSES and IBL_PATH_AUTO give the per-layer kernels.  The parameters are judged before the
 *   graph, so these refusals need no device.  The fused on-chip kernel of this arithmetic has an entry point of its
 *   own, ibl_layered_create_fixed_fused (below); this function never chooses it.
 *   Layout: a lane owns 4 consecutive codewords and a wave updates one check for 256.  The handle owns, allocated at
 *   create for ldb = max_batch rounded up to 256 codewords, the APP values [N][ldb] int8 and ONE 32-bit state word
 *   per check and codeword [n_c][ldb] (corrected m2 << 26 | corrected m1 << 20 | first argmin position << 16 | the
 *   sign bits of R, edge k at bit k), and, per 64 codewords as on the fp32 per-layer path, the packed hard decisions
 *   (one bit per variable and codeword), a 64-bit mask of finished and one of unsatisfied codewords, and a counter:
 *   memory  N ldb + 4 n_c ldb + 8 N ceil(max_batch / 64) + 64 ldb / 256 + 4  bytes, about N + 4 n_c + N / 8 per
 *   codeword (DVB-S2 N = 64800 rate 1/2: 202.5 KB per codeword, 1.66 GB at 8192, against 5.3 GB in fp32).  An
 *   iteration moves 2 E + 8 n_c bytes per codeword (fp32: 8 E + 24 n_c).
 *   A WIDE handle (a check of degree above 16; ibl_layered_is_wide) keeps TWO 32-bit words per check and codeword,
 *   for every check of its code, in two arrays [n_c][ldb] — word 0 = corrected m2 << 11 | corrected m1 << 5 | first
 *   argmin position (5 bits), word 1 = the sign bits of R, edge k at bit k — a lane's four codewords one 16-byte
 *   access per array:  memory  N ldb + 8 n_c ldb + ...  as above, about N + 8 n_c + N / 8 bytes per codeword; an
 *   iteration moves 2 E + 16 n_c bytes per codeword.  Its staging and layer launches are kernels of their own;
 *   everything else, the launch chain included, is as for a narrow handle.
 *   ibl_layered_decode on such a handle takes llr_dtype and out_dtype in {IBL_F32, IBL_I8} in any combination
 *   (anything else is IBL_EINVAL); d_out may be d_llr when the dtypes match.  It enqueues the launch chain of the
 *   fp32 per-layer path (staging, n_layers launches per iteration, pack / syndrome / finalise after every iteration
 *   but the last when early_stop is set, output) with the same guarantees: no allocation, no host synchronisation,
 *   no read-back; finished and padding codewords store nothing that reaches the caller; a finished codeword's values
 *   are frozen at its stop iteration.
 * ibl_layered_create_fixed_fused  the same arithmetic, bit for bit, in the fused on-chip form of the fp32 decoder: one
 *   wave owns one codeword in LDS through all iterations, one launch per decode, and a wave whose codeword's syndrome
 *   is zero takes its next codeword at once.  Validation as ibl_layered_create_fixed, the parameters before the
 *   graph: out-of-range alpha16 / beta_q / q_max / scale, imax or max_batch < 1 and a NULL out are IBL_EINVAL, then
 *   "graph is NULL", then the layers.
 *   Fit rule: a codeword occupies  cw_bytes = ldn + 4 n_c  bytes of LDS (wide: ldn + 8 n_c), ldn = N rounded up to a
 *   multiple of 4, and a workgroup keeps  cw_per_group = min(4, floor(160 KiB / cw_bytes))  codewords, one wave
 *   each (WLAN N = 1944: 5,832 bytes, 28 would fit; N = 16200, n_c = 9000: 52,200 bytes, 3 codewords, where the fp32
 *   fused kernel's 172,800 do not fit).  cw_per_group = 0 is IBL_EUNSUPPORTED with cw_bytes and the 160 KiB in the
 *   message (DVB-S2 N = 64800: use ibl_layered_create_fixed).  Several workgroups share a CU, so the cap of 4 costs
 *   no occupancy; IBL_LAYFIX_FUSED_CW = 1..16 in the environment at create replaces it (a measurement aid).
 *   LDS layout of a wave's slice: P[ldn] int8 APP values, then S[n_c], the state word of ibl_layered_create_fixed;
 *   a wide handle has S[n_c] then S1[n_c], its two state words.  P is read and written with byte accesses.
 *   Memory owned: the fp32 fused decoder's device plan (4 words per task, 64 variable indices per task and edge
 *   position) and a [max_batch][ldn] int8 staging buffer; nothing per check and codeword in device memory.
 *   ibl_layered_decode on such a handle takes llr_dtype and out_dtype in {IBL_F32, IBL_I8} in any combination
 *   (anything else is IBL_EINVAL; B > max_batch is IBL_EINVAL); d_out may be d_llr when the dtypes match.  It
 *   enqueues THREE launches at any imax — stage-in (64 x 64 tile transpose into the staging buffer, quantising
 *   IBL_F32 or copying IBL_I8 with -128 -> -127), the fused kernel, stage-out (transpose back, int8 or
 *   f32(P) / f32(scale)) — with no allocation, no host synchronisation and no read-back: capturable.
 *   ibl_layered_path_in_use gives 1, ibl_layered_is_fixed 1, ibl_layered_is_wide as for any handle,
 *   ibl_layered_geometry the real (cw_per_group, ngroups, grid); ibl_layered_set_compaction and
 *   ibl_layered_compaction_stats refuse with IBL_EUNSUPPORTED.
 * ibl_layered_is_fixed  *fixed = 1 for a handle of ibl_layered_create_fixed or _fixed_fused, 0 otherwise.
 */
int ibl_layered_create_fixed(const ibl_graph* g, int32_t n_layers, const int32_t* layer_ptr,
                             const int32_t* layer_checks, int32_t imax, int32_t alpha16, int32_t beta_q, int32_t q_max,
                             float scale, int32_t max_batch, int32_t path, ibl_layered** out);
int ibl_layered_create_fixed_fused(const ibl_graph* g, int32_t n_layers, const int32_t* layer_ptr,
                                   const int32_t* layer_checks, int32_t imax, int32_t alpha16, int32_t beta_q,
                                   int32_t q_max, float scale, int32_t max_batch, ibl_layered** out);
int ibl_layered_is_fixed(const ibl_layered* h, int32_t* fixed);

/*
 * Error counter.  Replaces return_errors_all_zero (discrete_LDPC_decoder_irreg.py:343-349,
 * discrete_LDPC_decoder.py:297-300, min_sum_decoder_irreg.py:290-295): counts entries
 * x[r][b] < threshold for r < rows, b < B (row stride ld) into the device int64 *d_count
 * (overwritten).  IB: threshold = T_dec/2; float: threshold = 0.
 */
int ibl_count_below(const void* d_x, int32_t dtype, int64_t rows, int32_t B, int64_t ld, double threshold,
                    int64_t* d_count, void* stream);

/* Channel generation on the device — replaces
 * AWGN_Channel_Transmission/AWGN_Quantizer_BPSK.py quantize_direct_OpenCL (:216-240) and
 * quantize_direct_OpenCL_LLR (:242-260) + kernels_quanti_template.cl (:1-52), which sample
 * u ~ U[0,1) with np.random.rand on the host and upload N*B float64 per batch.
 *
 * Writes out[r][b] (row stride ld elements, r < n, b < B) for the quantiser with cluster CDF
 * cdf[0..T] (host array, cdf[0] = 0, T <= 64): t = #{w in 1..T : u > cdf[w]} clamped to T-1,
 * mirrored to T-1-t where d_bits[r*B+b] is 1 (d_bits may be NULL: all-zero codeword).
 * out_dtype IBL_U8 / IBL_I32 store t; IBL_F32 / IBL_F64 store llr[t] (host array of T).
 * u for element i = r*B+b is the i-th output x of numpy's np.random.Philox(counter=offset,
 * key=seed) stream as (x >> 11) * 2^-53; a batch consumes ceil(n*B/4) counter blocks, so the
 * next batch (or GPU) uses offset += ceil(n*B/4).
 */
int ibl_channel_sample(const double* cdf, int32_t T, const double* llr, uint64_t seed, uint64_t offset, int32_t n,
                       int32_t B, const uint8_t* d_bits, void* d_out, int32_t out_dtype, int64_t ld, void* stream);

/* ---- LDPC encoding ------------------------------------------------------
 * Batched systematic encoder, replacing Discrete_LDPC_decoding/LDPC_encoder.py: the plan that
 * getLDPCEncoderParamters (:197-269) derives from H = [A | B] (B triangular with a full diagonal,
 * possibly after reversing its rows -> forward/backward substitution; else GF(2) factorisation
 * gf2factorize :287-340 with its first-candidate pivot rule -> "Matrix Inverse") is built natively
 * from H's canonical CSR (sorted columns); encode (:86-123) / encode_c (:125-162) run for B
 * codewords at once, 32 codewords per dword. A bidiagonal substitution (DVB-S2 IRA parity) runs as a
 * segmented prefix-XOR scan. Returns IBL_EINVAL when B is singular in GF(2) (the reference raises).
 */
typedef struct ibl_encoder ibl_encoder;
int ibl_encoder_create(int32_t n_v, int32_t n_c, const int32_t* indptr, const int32_t* cols, int32_t max_batch,
                       int32_t device, ibl_encoder** out);
/* "Forward Substitution" | "Backward Substitution" | "Matrix Inverse" (EncodingAlgorithm, :269) */
const char* ibl_encoder_algorithm(const ibl_encoder* h);
/* d_info: u8 [K][B] information bits (0/1), d_code: u8 [N][B] codewords [info; parity]
 * (LDPC_Transmitter.py transmit :109-125 encodes msg_at_time columns one by one). */
int ibl_encode(ibl_encoder* h, const uint8_t* d_info, int32_t B, uint8_t* d_code, void* stream);
void ibl_encoder_destroy(ibl_encoder* h);

/* Random information bits u8 [n][B] (np.random.randint(0, 2, (data_len, msg_at_time)) in
 * LDPC_Transmitter.py:111): bit i = top bit of the i-th 64-bit output of numpy's Philox4x64-10
 * stream with key (seed, 1) advanced by `offset` blocks
 * (Generator(Philox(key=seed + 2**64)).advance(offset).random_raw(n*B) >> 63); the next batch uses
 * offset += ceil(n*B/4). Key word 1 = 1 keeps the information bits disjoint from the channel stream
 * of ibl_channel_sample, whose key is (seed, 0), for any seed. */
int ibl_random_bits(uint64_t seed, uint64_t offset, int32_t n, int32_t B, uint8_t* d_out, void* stream);

/* Bit errors of decoder output against transmitted bits: *d_count = #{(r,b): r < rows, b < B,
 * (x[r*ld+b] < threshold) != (bits[r*bits_ld+b] != 0)} as int64 (generalises
 * return_errors_all_zero, Discrete_LDPC_decoding/discrete_LDPC_decoder_irreg.py:343-349, to non-zero codewords;
 * threshold T/2 for cluster ids, 0 for LLRs). x dtype: IBL_U8/IBL_I32/IBL_F32/IBL_F64. */
int ibl_count_errors(const void* d_x, int32_t dtype, int64_t rows, int32_t B, int64_t ld, double threshold,
                     const uint8_t* d_bits, int64_t bits_ld, int64_t* d_count, void* stream);

/* ---- Multi-GPU batch split without torch ------------------------------------------
 * The protocol of informationbottleneckdecodingldpc_amd/distributed.py for C / C++ callers: one process per
 * GPU; rank 0 builds H and the tables and broadcasts them once (ibl_comm_broadcast of the sizes, then of
 * each array — H's CSR and the LUT / matching vectors of ibl_ib_create); every rank decodes its contiguous
 * codeword range (ibl_shard_range) with its own ibl_graph / decoder; per Eb/N0 point one
 * ibl_comm_allreduce_sum_i64 of the counters {errors, bits, codewords}. No collective inside a decode (the
 * reference decodes on one OpenCL device and has no communication, discrete_LDPC_decoder_irreg.py:174-175).
 * Collectives run on RCCL (NCCL's API on ROCm, over xGMI), loaded at run time (dlopen librccl.so.1);
 * IBL_EUNSUPPORTED when it cannot be loaded.
 */
/* [start, start + count) of `rank`'s share of `total` codewords (contiguous, sizes differ by at most 1). */
int ibl_shard_range(int64_t total, int32_t rank, int32_t world, int64_t* start, int64_t* count);
#define IBL_COMM_ID_BYTES 128
typedef struct ibl_comm ibl_comm;
/* rank 0 creates the id (IBL_COMM_ID_BYTES bytes) and hands it to every rank out of band (MPI, a file, TCP) */
int ibl_comm_unique_id(uint8_t* id);
/* collective: every rank of `nranks` calls it with the same id, its rank and its device */
int ibl_comm_create(const uint8_t* id, int32_t nranks, int32_t rank, int32_t device, ibl_comm** out);
/* d_buf: device memory of `bytes` bytes on the communicator's device; asynchronous on `stream` */
int ibl_comm_broadcast(ibl_comm* c, void* d_buf, int64_t bytes, int32_t root, void* stream);
/* in-place sum over ranks of `count` int64 device values; asynchronous on `stream` */
int ibl_comm_allreduce_sum_i64(ibl_comm* c, int64_t* d_buf, int64_t count, void* stream);
void ibl_comm_destroy(ibl_comm* c);

#ifdef __cplusplus
}
#endif

#endif /* IBLDPC_H */
