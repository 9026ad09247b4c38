/*
 * flowtron_hip.h -- C ABI of libflowtron_hip.so (MI355X / gfx950 only).
 *
 * The reference (NVIDIA/flowtron) has no FFI: its only boundary is the Python
 * module API (flowtron.py Flowtron.forward/infer, audio_processing.py
 * TacotronSTFT, distributed.py).  This header is the boundary a maintainer
 * binds instead of the PyTorch/cuDNN/cuBLAS op call sites listed below; the
 * ctypes stub that does it is flowtron_amd/_lib.py.
 *
 * Conventions
 *   - every entry point returns 0 on success, a negative FT_E* code on error;
 *     ft_last_error() returns a thread-local message for the last failure.
 *   - all buffers are caller-owned DEVICE pointers (fp32 unless stated);
 *     the library never allocates, frees or retains them.  Lengths are device
 *     int32 arrays.  No entry point synchronises: work is enqueued on `stream`
 *     (a hipStream_t passed as void*), in order, and is hipGraph-capturable.
 *   - `mode` selects the MFMA operand type of matmul-shaped work:
 *     FT_F32 = fp32 operands (v_mfma_f32_16x16x4_f32, exact fp32, parity mode),
 *     FT_BF16 = operands rounded to bf16 on the way into the matrix core
 *     (v_mfma_f32_16x16x32_bf16), fp32 accumulate.  Storage stays fp32.
 *     FT_F16 = the same code path with fp16 operands (v_mfma_f32_16x16x32_f16):
 *     the reference's fp16 AMP configuration (train.py:254,292).  Values beyond
 *     65504 round to +-inf, which is what torch's GradScaler inf check expects.
 *     Entry points with a `mode` argument accept FT_F16 directly; the ones that
 *     consume or produce 16-bit images / fragments without a mode argument have
 *     a twin of identical signature and the suffix _f16 (end of this header).
 *   - time-major activations: [T,B,C] row-major, like the reference's
 *     internal layout after flowtron.py:884.
 *
 * Where this header departs from the conventions SURVEY.md 8(b) sketched (the
 * reference itself has no FFI to be compatible with; these are choices):
 *   - no `ft_ctx` handle with create / destroy entry points: the library keeps NO
 *     per-device state.  Every entry point works on the device of the stream it
 *     is handed (the caller -- torch -- has made it current); scratch, status
 *     words and weight images are caller-owned buffers passed per call, so the
 *     library is re-entrant across devices and processes by construction.
 *   - positional arguments instead of one args struct per op, except where an op
 *     has more than ~12 operands (ft_gemm, ft_gemm_img, ft_decode_flow,
 *     ft_cumm_attn_*: structs).
 *   - no `ft_allreduce_flat`: the gradient exchange is torch.distributed's RCCL
 *     all-reduce of the flat arena (north_star: "a single RCCL all-reduce over
 *     xGMI per step"; flowtron_amd/dist.py); the library only supplies the
 *     device-side poison / non-finite-norm guard around it.
 *   - `ft_dense_conv_affine` (dense -> dense -> 1x1 conv -> coupling as ONE
 *     kernel) is not built: a 1024-wide layer pair per row tile needs both weight
 *     matrices (4 MB of 16-bit operands) per tile from the L2 -- 2.6 GB per
 *     call at 32-row tiles, the largest that keep two activation tiles in LDS --
 *     which is slower than the three image GEMMs it would replace.  What IS fused:
 *     bias + tanh in the GEMM epilogue, the activation backward + bias gradient
 *     in the gradient's image pass (ft_bf16_image_rows_act_bwd), the coupling
 *     with its own backward (ft_affine_*), the masked NLL sums (ft_masked_sum).
 *   - `ft_decode_init` / `ft_decode_steps` became ft_decode_flow (one call per
 *     flow: a persistent launch, or a hipGraph of staged frames).
 *   - `ft_lstm_seq` "multi-layer": one call per layer (ft_lstm_persist_* /
 *     ft_lstm_seq_*), with the inter-layer projection as a batched GEMM between
 *     them (faster than the fused two-layer wavefront, which is kept as
 *     ft_lstm2_seq_* for shapes the persistent kernels do not take).
 */
#ifndef FLOWTRON_HIP_H
#define FLOWTRON_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FT_ABI_VERSION 15
/* (ft_gemm_img_args grew its trailing a_rows field and ft_chunk_gather_rows was added WITHOUT a new number: 14 therefore names two struct
 * layouts, and a caller's ft_abi_version() check cannot tell a library built before the field from one built after it.  Callers zero-
 * initialise the struct and are built together with the library (flowtron_amd/build.py rebuilds on any header change); a binding kept
 * outside this tree must be rebuilt against this header.)
 * 15: ft_gemm_img_plan. */

enum { FT_OK = 0, FT_EINVAL = -1, FT_EHIP = -2, FT_EUNSUPPORTED = -3 };
enum { FT_F32 = 0, FT_BF16 = 1, FT_F16 = 2 };
enum { FT_ACT_NONE = 0, FT_ACT_TANH = 1, FT_ACT_RELU = 2, FT_ACT_SIGMOID = 3 };
enum { FT_GEMM_SPLITK = 1, FT_GEMM_SPLITK_DET = 2, FT_GEMM_C16 = 4 };   /* FT_GEMM_C16 (ABI 13, ft_gemm_img only): C is a 16-bit matrix of the
 * call's operand format (bf16; fp16 for the _f16 twin), ldc in 16-bit elements, beta = 0, no split-K: what the persistent forward recurrence reads as gx */

int ft_abi_version(void);
const char* ft_last_error(void);
/* test hook: n_wg workgroups that each hold a whole CU for `ticks` of the 100 MHz wall clock (clamped to 5 s) on `stream` -- a
 * stand-in for a foreign kernel (an in-flight collective) beside a whole-chip persistent launch (tests/test_gpu_dist.py) */
int ft_debug_hold_cus(int n_wg, int64_t ticks, void* stream);

/* ---- GEMM ---------------------------------------------------------------
 * C[b][m][n] = act( alpha * sum_k A[b](m,k) * B[b](k,n) + beta * C[b][m][n] + bias[n] )
 * A(m,k) = A[b*bsA + m*sAm + k*sAk],  B(k,n) = B[b*bsB + k*sBk + n*sBn],
 * C row-major with leading dimension ldc.  Replaces every nn.Linear / Conv1d /
 * torch.bmm call site of the hot path: flowtron.py:568-571 (Q/K/V), :590 (context),
 * :758 (gate), :767-768 (dense, 1x1 conv), the LSTM input projections inside
 * nn.LSTM (:654-655, :488), the encoder Conv1d (:479-483, as im2col GEMM) and
 * their autograd-derived transposes. */
typedef struct {
    const float* A; const float* B; float* C; const float* bias;
    int M, N, K, batch;
    int64_t sAm, sAk, sBk, sBn, ldc;
    int64_t bsA, bsB, bsC;
    float alpha, beta;
    int act, mode;
    int flags;   /* FT_GEMM_SPLITK: allow split-K with fp32 atomics when the output has few tiles and K is long (weight
                  * gradients over T*B rows).  Summation order is then not reproducible bit-for-bit, so the forward path
                  * never sets it. */
    void* work;  /* optional scratch (256-byte aligned) of ft_gemm_workspace_bytes() bytes.  When given (FT_BF16, batch 1,
                  * problem large enough for the query to be non-zero) the operands are first rewritten once as zero-padded
                  * bf16 images with the reduction dimension innermost and the GEMM runs from those through direct
                  * global->LDS DMA; same rounding (RNE to bf16, fp32 accumulate) as the staging path taken when it is NULL. */
    size_t work_bytes;
} ft_gemm_args;
size_t ft_gemm_workspace_bytes(const ft_gemm_args* a);
int ft_gemm(const ft_gemm_args* a, void* stream);

/* bf16 operand images (FT_BF16 training path): a row-major fp32 matrix [rows][cols] (row stride ld) is rounded ONCE to a
 * zero-padded bf16 image [ceil256(rows + 32)][ceil256(cols)] (ft_bf16_image_bytes bytes, 256-byte aligned) and then feeds
 * every GEMM that reads it, in either role:
 *   k-contiguous operand (a_kmajor / b_kmajor = 0): image rows are the operand's m (or n) index, columns the reduction;
 *   k-major operand (= 1): image rows are the reduction index, columns the m (or n) index -- read through the LDS
 *   transpose-read, so the weight-gradient GEMMs dW = dY^T X (both operands k-major) need no transposed copies.
 * A / B may point INSIDE an image (row offset * ld for a time shift, column offset % 8 == 0 for a column block of a
 * weight); whatever lies beyond the logical extent must be finite and is multiplied by the partner's zero padding (k) or
 * dropped by the epilogue (m, n).  lda / ldb = image row stride in elements = ceil256(cols).  Epilogue as ft_gemm. */
typedef struct {
    const void* A; const void* B; float* C; const float* bias;
    int M, N, K;
    int64_t lda, ldb, ldc;
    int a_kmajor, b_kmajor;
    float alpha, beta;
    int act, flags;
    /* compact row space (pack-by-length, the reference's pack_padded_sequence at flowtron.py:689-694): the images were made by
     * ft_bf16_image_rows from the VALID rows only.  compact = 0: plain.  1: the M rows are compact rows -- workgroup tiles at or
     * beyond *rows_dev exit at once, and compact row m is written to C row rowmap[m] (negative: dropped); M = the capacity the
     * grid is sized for; no split-K.  2: the reduction runs over compact rows -- K = capacity, k-steps at or beyond
     * *rows_dev - k_shift are not visited (k_shift = the row offset already applied to A for a one-step time shift). */
    const int32_t* rowmap; const int32_t* rows_dev;
    int compact, k_shift;
    /* optional rank-1 epilogue term (ABI 10): C[row][col] += r1_row[row] * r1_col[col] in fp32, row = the OUTPUT row (after the
     * row map), before the activation; both NULL = none; not with split-K.  The gate layer's input gradient dgate (x) w_gate rides
     * on the decoder input projection's dX GEMM this way (flowtron.py:758-761: both read [h_att ; ctx]). */
    const float* r1_row; const float* r1_col;
    /* deterministic split-K (ABI 12; flags & FT_GEMM_SPLITK_DET, beta = 0, no activation, compact = 0, N % 4 == 0): the k-slices
     * write their partial products side by side into split_work (ft_gemm_img_split_work_bytes(M, N, K) bytes, 16-byte aligned) with
     * plain stores and a second kernel adds them in ascending slice order (+ bias): the result is a function of the operands, which
     * the fp32 atomics of FT_GEMM_SPLITK are not (their order varies from run to run).  For FORWARD GEMMs with few output tiles and
     * a long reduction (the encoder convolutions' split-image product, flowtron.py:499-502); NULL / 0: never splits. */
    void* split_work; size_t split_work_bytes;
    /* optional row gather of A (device list, NULL = none): with compact = 1, a_kmajor = 0, no split-K flag and K % 64 == 0 (anything else:
     * FT_EINVAL) compact row m < *rows_dev reads image row a_rows[m] of A instead of row m; the rows of the last tile at or beyond
     * *rows_dev read row a_rows[*rows_dev - 1] (their outputs are dropped), so A need not hold zeros anywhere.  Same k order as the plain
     * call: the result equals that of an image whose rows were gathered beforehand, bit for bit.  The decoder pair's backward pipeline
     * reads the rows of ONE time chunk out of the batch-major dgates image this way (ft_chunk_gather_rows). */
    const int32_t* a_rows;
} ft_gemm_img_args;
size_t ft_gemm_img_split_work_bytes(int M, int N, int K);
/* ABI 15: what ft_gemm_img(a) / ft_gemm_img_f16(a) would launch, decided by the launcher's own code -- no launch, no device access (the
 * pointers are only looked at for NULL and alignment).  Same return codes as the call itself for arguments it would refuse.  One of the
 * tile forms of the kernel: tile_rows x 128 outputs per workgroup; stage_k = 64: the single-buffer form with 64-wide k stages; gather: A's
 * rows through a_rows; atomics: split-K with fp32 atomics; det: split-K through split_work and the fixed-order reduction; splits = k-slices
 * launched (compact = 2: the kernel divides the rows the batch has over them); chunk_w > 0: the L2-aware tile order with column chunks of
 * that many tiles.  Lets a test assert which path a shape reaches. */
typedef struct { int tile_rows;      /* 128 | 256 */
                 int stage_k;        /* 32 | 64 (64 = single-buffer form) */
                 int gather, atomics, det, splits, chunk_w; } ft_gemm_img_plan_t;
int ft_gemm_img_plan(const ft_gemm_img_args* a, ft_gemm_img_plan_t* out);
/* Grouped weight-gradient GEMMs (added under ABI 15: a new entry point, nothing existing changes).  n (1 .. 48) problems, each the
 * ft_gemm_img_args of a weight-gradient call -- a_kmajor = b_kmajor = 1, no activation, beta 0 or 1, optional bias (added once), compact
 * 0 or 2 with rows_dev / k_shift, fp32 C of any ldc, FT_GEMM_SPLITK to allow k-slices (K >= 2048) -- run in ONE grid per tile height
 * (256-row tiles where M >= 512, else 128): a workgroup is one (problem, tile, k-slice).  The planner cuts every problem of a launch
 * into slices of near-equal length that fill whole rounds of the chip's workgroup slots with as few slices as that takes, longest
 * first; a problem with ONE slice whose C overlaps no other problem's C is written with plain loads and stores, the others add with
 * fp32 atomics (beta = 0: C is cleared first).  Anything else in a problem: FT_EINVAL, nothing is launched.  probs is a HOST array.
 * The plan query reports, per problem in the caller's order: the tile height, the k-slices and their length in 32-wide k-steps (compact
 * = 2: the kernel divides the rows the batch has over the slices instead), atomics (0 = plain stores), the launch (0 = first) and
 * the problem's first unit and tile count in it: unit u of the problem is k-slice u / tiles of tile u % tiles.  No launch, no device access. */
typedef struct { int tile_rows, splits, ksteps, atomics, launch, unit0, tiles; } ft_gemm_img_group_plan_t;
int ft_gemm_img_group_plan(const ft_gemm_img_args* probs, int n, ft_gemm_img_group_plan_t* out);
int ft_gemm_img_group(const ft_gemm_img_args* probs, int n, void* stream);
size_t ft_bf16_image_bytes(int64_t rows, int64_t cols);
int ft_bf16_image(const float* src, int64_t ld, int64_t rows, int64_t cols, void* dst, void* stream);
/* the same image plus colsum[c] = sum_r src[r][c] in fp32 (bias gradients ride on the conversion pass of the output
 * gradient; colsum [cols] is overwritten; row slabs combine with fp32 atomics like ft_colsum) */
int ft_bf16_image_colsum(const float* src, int64_t ld, int64_t rows, int64_t cols, void* dst, float* colsum, void* stream);
int ft_gemm_img(const ft_gemm_img_args* a, void* stream);
/* _acc forms (ABI 12) of the three image passes that also produce column sums (ft_bf16_image_colsum, ft_bf16_image_rows with a colsum,
 * ft_bf16_image_rows_act_bwd): the sums are ADDED to colsum, which the caller has zeroed (a slice of one zeroed slab per backward
 * pass) -- the plain forms clear it with a memset dispatch of their own, 11 per training step. */
int ft_bf16_image_colsum_acc(const float* src, int64_t ld, int64_t rows, int64_t cols, void* dst, float* colsum, void* stream);
int ft_bf16_image_rows_acc(const float* src, int64_t ld, int64_t cap_rows, int64_t cols, void* dst, float* colsum,
                           const int32_t* rowmap, const int32_t* rows_dev, void* stream);
int ft_bf16_image_rows_act_bwd_acc(const float* dy, int64_t ld, const float* y, int64_t ldy, int act, int64_t cap_rows, int64_t cols,
                                   void* dst, float* colsum, const int32_t* rowmap, const int32_t* rows_dev, void* stream);
int ft_bf16_image_colsum_acc_f16(const float* src, int64_t ld, int64_t rows, int64_t cols, void* dst, float* colsum, void* stream);
int ft_bf16_image_rows_acc_f16(const float* src, int64_t ld, int64_t cap_rows, int64_t cols, void* dst, float* colsum,
                               const int32_t* rowmap, const int32_t* rows_dev, void* stream);
int ft_bf16_image_rows_act_bwd_acc_f16(const float* dy, int64_t ld, const float* y, int64_t ldy, int act, int64_t cap_rows, int64_t cols,
                                       void* dst, float* colsum, const int32_t* rowmap, const int32_t* rows_dev, void* stream);
/* Split images (ABI 11): x = hi + lo, hi = op16(x), lo = op16(x - hi).  dst = [rows][3 cols] 16-bit (ft_bf16_image_bytes(rows, 3 cols),
 * row stride ceil256(3 cols)): an activation (weight = 0) as [hi | lo | hi], a weight matrix (weight = 1) as [hi | hi | lo], so that ONE
 * ft_gemm_img with K = 3 cols computes x_hi w_hi + x_lo w_hi + x_hi w_lo = x . w to ~2^-17 -- fp32-grade products at three times a
 * 16-bit GEMM's cost.  Used for the FORWARD of the encoder's convolutions (flowtron.py:499-502): their 16-bit rounding, renormalised
 * by the instance norm behind them, was the source of the 0.11 relative deviation of the text-embedding gradient in bf16 training
 * (measured round 5: fp32 forward products alone bring it to 0.008).  cols % 8 == 0. */
int ft_bf16_image_split3(const float* src, int64_t ld, int64_t rows, int64_t cols, void* dst, int weight, void* stream);
int ft_bf16_image_split3_f16(const float* src, int64_t ld, int64_t rows, int64_t cols, void* dst, int weight, void* stream);
/* ABI 14: the split ACTIVATION image of the im2col matrix of ft_im2col(x, lens, L, B, C, KW) -- [L * B rows][3 * C * KW] as [hi | lo | hi] --
 * made straight from x [L][B][C] (flowtron.py:499-502: the encoder convolution as a GEMM): the fp32 column matrix is never written.
 * dst: ft_bf16_image_bytes(L * B, 3 * C * KW) bytes; (C * KW) % 8 == 0, KW odd. */
int ft_bf16_image_split3_im2col(const float* x, const int32_t* lens, int L, int B, int C, int KW, void* dst, void* stream);
int ft_bf16_image_split3_im2col_f16(const float* x, const int32_t* lens, int L, int B, int C, int KW, void* dst, void* stream);
/* The weight images of one forward pass in ONE launch (ABI 12): descs = HOST array of n <= 32 descriptors, kind 0 = what
 * ft_bf16_image(src, ld, rows, cols, dst) writes, kind 1 = ft_bf16_image_split3(src, ld, rows, cols, dst, weight = 1).  A training step
 * rounds its 23 weight matrices afresh every iteration; one dispatch instead of 23 of 5-15 us each. */
typedef struct { const float* src; int64_t ld; int64_t rows; int64_t cols; void* dst; int kind; } ft_img_desc;
int ft_bf16_image_table(const ft_img_desc* descs, int n, void* stream);
int ft_bf16_image_table_f16(const ft_img_desc* descs, int n, void* stream);
/* Pack-by-length row map of a time-major [T][B][*] activation (flowtron.py:689-694 packs, here without a host sync): compact
 * rows are batch-major -- utterance b contributes rows (t, b), t < lens[b], then ONE separator: row (lens[b], b) when
 * lens[b] < T (the utterance's first padded frame, which stands for all of them: every padded frame of b holds the same
 * values), else -1 (a zero row).  rowmap needs T*B + B entries; rows_dev[0] = sum_b (lens[b] + 1).  The separator rows make the
 * one-step shift of the recurrent weight gradient (dW_hh = sum_t dgates_t^T h_{t-1}) a one-ROW shift in compact space. */
int ft_rowmap_build(const int32_t* lens, int32_t* rowmap, int32_t* rows_dev, int T, int B, void* stream);
/* The row lists of the time chunk [t0, t1) of that batch, for a GEMM over the chunk's rows that reads them out of the WHOLE sequence's
 * compact image (ft_gemm_img_args.a_rows): the chunk's compact rows are ft_rowmap_build's over the lengths clamp(lens[b] - t0, 0, t1 - t0)
 * (so *rows_dev is that map's).  Compact row i = (t, b), t local to the chunk: a_rows[i] = off_b + t0 + t with off_b = sum over b' < b of
 * (lens[b'] + 1), rowmap[i] = t * B + b.  The chunk's separator rows are dropped (rowmap -1) and read a valid row of the chunk: the image's
 * own separator rows need not have been written yet.  Both lists need (t1 - t0) * B + B entries. */
int ft_chunk_gather_rows(const int32_t* lens, int32_t* a_rows, int32_t* rowmap, int T, int B, int t0, int t1, void* stream);
/* compact image: image row i = bf16(src row rowmap[i]) for i < *rows_dev (negative: zeros), zeros up to
 * ceil256(*rows_dev + 32); dst holds ft_bf16_image_bytes(cap_rows, cols).  colsum (optional) as ft_bf16_image_colsum. */
int ft_bf16_image_rows(const float* src, int64_t ld, int64_t cap_rows, int64_t cols, void* dst, float* colsum,
                       const int32_t* rowmap, const int32_t* rows_dev, void* stream);
/* The output gradient of an ACTIVATED dense layer (tanh / relu / sigmoid fused in ft_gemm_img's epilogue, flowtron.py:453-464)
 * straight into its operand image: dst = image(dy * act'(pre)) over the compact rows of `rowmap`, act' through the saved output
 * y = act(pre) like ft_act_bwd; colsum [cols] = the bias gradient.  Replaces ft_act_bwd + ft_bf16_image_rows. */
int ft_bf16_image_rows_act_bwd(const float* dy, int64_t ld, const float* y, int64_t ldy, int act, int64_t cap_rows, int64_t cols,
                               void* dst, float* colsum, const int32_t* rowmap, const int32_t* rows_dev, void* stream);
int ft_bf16_image_rows_act_bwd_f16(const float* dy, int64_t ld, const float* y, int64_t ldy, int act, int64_t cap_rows, int64_t cols,
                                   void* dst, float* colsum, const int32_t* rowmap, const int32_t* rows_dev, void* stream);
/* One column block of a compact image: src [*, cols] -> columns [col_off, col_off + cols) of dst (row stride dst_ld elements; the
 * image is sized by ft_bf16_image_bytes for its TOTAL width), columns up to col_off + fill_cols zeroed.  A Linear over two
 * inputs ([h_att ; ctx] W^T, flowtron.py:758-765) then runs as ONE GEMM over one image instead of two K pieces. */
int ft_bf16_image_rows_into(const float* src, int64_t ld, int64_t cap_rows, int64_t cols, void* dst, int64_t dst_ld, int64_t col_off,
                            int64_t fill_cols, const int32_t* rowmap, const int32_t* rows_dev, void* stream);
int ft_bf16_image_rows_into_f16(const float* src, int64_t ld, int64_t cap_rows, int64_t cols, void* dst, int64_t dst_ld, int64_t col_off,
                                int64_t fill_cols, const int32_t* rowmap, const int32_t* rows_dev, void* stream);
/* N = 1 projection over a compact image (the gate layer LinearNorm(n_hidden + n_attn, 1), flowtron.py:668-669 / :760-761, reads the
 * rows the decoder LSTM's input projection has just multiplied): y[rowmap[c]] = sum_k img[c][k] * op16(w[k]) + bias[0] for the compact
 * rows c < *rows_dev; y = [T*B] rows of stride ldy; every padded frame of an utterance receives its separator's value.  The image
 * must be zero from column K up to the next multiple of 8 (ft_bf16_image_rows / _into pad with zeros).
 * _bwd: dw[k] += sum_c dy[rowmap[c]] img[c][k], db[0] += sum_c dy[rowmap[c]] (db may be NULL); dw / db ACCUMULATE: the caller zeroes. */
int ft_img_gemv_rows(const void* img, int64_t ld, int K, const float* w, const float* bias, float* y, int64_t ldy,
                     const int32_t* rowmap, const int32_t* rows_dev, const int32_t* lens, int T, int B, void* stream);
int ft_img_gemv_rows_f16(const void* img, int64_t ld, int K, const float* w, const float* bias, float* y, int64_t ldy,
                         const int32_t* rowmap, const int32_t* rows_dev, const int32_t* lens, int T, int B, void* stream);
int ft_img_gemv_rows_bwd(const void* img, int64_t ld, int K, const float* dy, int64_t lddy, float* dw, float* db,
                         const int32_t* rowmap, const int32_t* rows_dev, int64_t cap_rows, void* stream);
int ft_img_gemv_rows_bwd_f16(const void* img, int64_t ld, int K, const float* dy, int64_t lddy, float* dw, float* db,
                             const int32_t* rowmap, const int32_t* rows_dev, int64_t cap_rows, void* stream);
/* rows (t, b) with t > lens[b] of the time-major matrix y [T*B][cols] (row stride ld): mode 0 = zero them, 1 = copy row
 * (lens[b], b) into them (a compact GEMM wrote only valid rows and the separator; consumers that walk every frame need the rest) */
int ft_pad_rows_fill(float* y, int64_t ld, int cols, const int32_t* lens, int T, int B, int mode, void* stream);

/* ---- embedding gather (flowtron.py:873-874) ------------------------------
 * out[r][0:dim] = W[ids[r]] for r < n (out row stride ld_out).  bwd: dW[ids[r]] += dout[r]. */
int ft_embedding_fwd(const int64_t* ids, const float* W, float* out, int n, int dim, int64_t ld_out, void* stream);
int ft_embedding_bwd(const int64_t* ids, const float* dout, float* dW, int n, int dim, int64_t ld_dout, void* stream);
/* The same sums with the rows walked at a stride (row r = i * stride + j): a thread adds its rows in a register while the id stays
 * the same and sends one atomic per run.  For ids that repeat with period `stride` -- the speaker embedding gathered for every text
 * position of a [L,B] batch (flowtron.py:886-887): stride = B -- that is 1 / 32 of the atomics; correct for ANY ids.  (ABI 12) */
int ft_embedding_bwd_runs(const int64_t* ids, const float* dout, float* dW, int n, int dim, int64_t ld_dout, int stride, void* stream);

/* ---- encoder conv as im2col (flowtron.py:499-502) --------------------------
 * x [L,B,C] time-major (must already be zero at l >= lens[b]);
 * col[l][b][c*KW + k] = x[l + k - KW/2][b][c] (0 outside [0,lens[b])).
 * col2im is the adjoint (gather form, deterministic). */
int ft_im2col(const float* x, float* col, const int32_t* lens, int L, int B, int C, int KW, void* stream);
int ft_col2im(const float* dcol, float* dx, const int32_t* lens, int L, int B, int C, int KW, void* stream);

/* ---- masked instance norm + ReLU (+dropout keep-mask) (flowtron.py:53-92, :502)
 * x,y [L,B,C]; statistics over l < lens[b] (biased variance, eps); y = relu(xhat*gamma+beta)*keep,
 * y = 0 at l >= lens[b].  keep may be NULL.  Saves mean/rstd [B,C] for backward.
 * bwd: dx (0 at pads), dgamma/dbeta [C] (overwritten).
 * lens[b] beyond L counts as L.  A sample with lens[b] <= 0 has y = 0 and dx = 0 everywhere and adds nothing to dgamma / dbeta; its
 * mean / rstd entries are not defined (0 / 0) and bwd, their only reader, does not use them. */
int ft_instnorm_relu_fwd(const float* x, const float* gamma, const float* beta, const float* keep,
                         const int32_t* lens, float* y, float* mean, float* rstd,
                         int L, int B, int C, float eps, void* stream);
int ft_instnorm_relu_bwd(const float* x, const float* y, const float* dy, const float* gamma, const float* keep,
                         const int32_t* lens, const float* mean, const float* rstd,
                         float* dx, float* dgamma, float* dbeta, int L, int B, int C, void* stream);

/* ---- length-masked LSTM over a whole sequence (nn.LSTM on a packed sequence:
 * flowtron.py:689-694 attention_lstm/lstm, :505-512 encoder BiLSTM) -----------------
 * gx [T,B,4H] = x W_ih^T + b_ih + b_hh (from ft_gemm); w_hh [4H,H], gate rows i|f|g|o.
 * Step s of sample b touches time t = s (forward) or lens[b]-1-s (reverse) while s < lens[b].
 * y [T,B,ldy] gets h_t at valid t and 0 at t >= lens[b].  gates [T,B,4H] (post-activation
 * i,f,g,o) and cell [T,B,H] are saved for backward.  work: ft_lstm_workspace_bytes() bytes.
 * bwd: dy [T,B,ldy] -> dgx [T,B,4H] (0 at pads); dW_hh/dW_ih/dx/db follow as ft_gemm /
 * ft_colsum calls over all T*B rows. */
size_t ft_lstm_workspace_bytes(int B, int H);
int ft_lstm_seq_fwd(const float* gx, const float* w_hh, const int32_t* lens,
                    float* y, int64_t ldy, float* gates, float* cell, void* work,
                    int T, int B, int H, int reverse, int mode, void* stream);
int ft_lstm_seq_bwd(const float* dy, int64_t ldy, const float* w_hh, const int32_t* lens,
                    const float* gates, const float* cell, float* dgx, void* work,
                    int T, int B, int H, int reverse, int mode, void* stream);

/* Persistent form of ft_lstm_seq_bwd (16-bit MFMA operands, H == 1024, B <= 32, 256-CU device): ONE launch for the whole sequence
 * (csrc/lstm_persist.hip, lstm_persist_bwd_rs_k).  The chip is split into 8 independent batch groups = the 8 XCDs, formed at run
 * time from the workgroups' XCC ids; every CU keeps the 16-bit MFMA fragments of its W_hh rows in registers for all T steps,
 * multiplies its OWN dgates with them and the fp32 partials are REDUCE-SCATTERED through the XCD's own L2, tagged in the mantissa LSB:
 * the same products as ft_lstm_seq_bwd(FT_BF16) in another, fixed association -- equal to fp32 rounding, deterministic.
 * `ng` = 21 (1 is accepted as "the default"); round 6 removed the all-gather transports 1 | 9 | 11 | 19 and the round-2..5 forward
 * kernel ft_lstm_persist_fwd / _fwd_rows / _bwd_rows: the forward recurrence and every batch wider than 32 run on ft_lstm_roles_* below.
 * `status` (device int32, zeroed by the caller once) is raised to 1 if a hand-off wait times out (grid not co-resident);
 * the caller must check it before trusting dgx.  work: ft_lstm_persist_workspace_bytes(), 256-byte aligned. */
int ft_lstm_persist_supported(int B, int H);
size_t ft_lstm_persist_workspace_bytes(int B, int H);
/* debug: device buffer [1024][4][5] int64 that subsequent ft_lstm_persist_bwd launches fill with per-step phase stamps
 * (100 MHz wall clock) of one workgroup; NULL switches it off. */
int ft_lstm_persist_debug_prof(void* dev_buf);
int ft_lstm_persist_bwd(const float* dy, int64_t ldy, const float* w_hh, const int32_t* lens, const float* gates,
                        const float* cell, float* dgx, void* work, int32_t* status, int T, int B, int H, int ng, void* stream);
/* The same launch, additionally leaving the 16-bit operand image of dgates in pack-by-length row order in `dimg` -- exactly what
 * ft_bf16_image_rows(dgx, ..., rowmap of `lens`) would produce afterwards (utterance b = its len_b frames + one zero separator
 * row, batch-major; zero rows up to ceil256(R + 32); dimg: ft_bf16_image_bytes(T*B + B, 4H), row stride dimg_ld elements,
 * dimg_rows rows allocated) -- and ADDING the column sums of dgates (the bias gradient of the layer) to dbias[4H] (zeroed by the
 * caller; fp32 atomics, one per workgroup row and column).  The weight- and input-gradient GEMMs (flowtron.py:689-694's
 * autograd transposes) then start without a conversion pass over the 450 MB dgx.  dgx == NULL: the image only. */
int ft_lstm_persist_bwd_img(const float* dy, int64_t ldy, const float* w_hh, const int32_t* lens, const float* gates,
                            const float* cell, float* dgx, void* work, int32_t* status, int T, int B, int H, int ng,
                            void* dimg, int64_t dimg_ld, int64_t dimg_rows, float* dbias, void* stream);

/* Round 6 (ABI 13): the persistent recurrences with the geometry as PARAMETERS (csrc/lstm_roles.hip) -- rows per XCD group R = 4 | 8 | 16
 * (an MFMA tile has 16 rows; the kernels above use 4), a time WINDOW [t0, t1) per launch with the recurrent state carried through
 * small fp32 buffers, and up to two ROLES (independent recurrences) per launch, role i on XCD groups i * 8 / n_roles .. (batch rows
 * <= (8 / n_roles) * R each).  What they replace is still cuDNN's nn.LSTM over packed sequences (flowtron.py:654-655, 689-694, 760-765):
 *   - a batch of 64 / 128 as ONE launch per sequence (n_roles 1, R 8 / 16) instead of 2 / 4 sliced launches;
 *   - the two decoder layers of a flow CONCURRENTLY, layer 1 one time chunk behind layer 0 (backward: the other way round), the chunk's
 *     input projection GEMM between the launches (flowtron_amd/ops.py DecoderPairFn).
 * wimg: MFMA fragment image of W_hh (ft_lstm_roles_wimg_bytes, 256-byte aligned), made once per pass by ft_lstm_roles_prepare_fwd / _bwd
 * (the backward image is the reduce-scatter layout).  ctx: launch context of ft_lstm_roles_ctx_bytes() bytes, 256-byte aligned,
 * initialised ONCE by ft_lstm_roles_ctx_init and then owned by the launches: `phase` = number of earlier launches of the same kind
 * (forward / backward) on this ctx -- a launch works in hand-off set phase & 1 and presets set (phase + 1) & 1 for `reset_rows` (>= the R
 * of the next launch of its kind) while it runs, so no preset dispatch precedes a launch.  Launches on one ctx must be serialised on
 * one stream.  `status` as for ft_lstm_persist_*.  Forward results are bit-identical to ft_lstm_seq_fwd for every R / windowing / role
 * placement; backward to fp32 rounding (R = 4: bit-identical to ft_lstm_persist_bwd's reduce-scatter transport).  A call in which EVERY
 * role's window is empty (t1 == t0) is refused with FT_EINVAL and launches nothing: it must not be counted in `phase` (a launch counted
 * that never ran would leave the next one in the wrong hand-off set).  One empty role beside a non-empty one is fine. */
typedef struct {
    const void* gx; const int32_t* lens; float* y; int64_t ldy; float* gates; float* cell;   /* as ft_lstm_seq_fwd; time steps ldb rows apart */
    const void* wimg;
    float* state_h; float* state_c;      /* [B][H] fp32: read when t0 > 0, written at the end of the window; NULL (both) for t0 == 0 without successor */
    int32_t B, ldb, t0, t1;
    int32_t gx16;                        /* 0: gx = fp32 rows [T][ldb][4H]; 1: 16-bit rows of the call's operand format (what ft_gemm_img writes with
                                          * FT_GEMM_C16: half the bytes; widened exactly before it is added to the fp32 recurrent sums) -- one format per launch */
    /* Trailing fields (appended without a new ABI number, like ft_gemm_img_args.a_rows: callers zero-initialise the struct).  xproj_k != 0:
     * there is NO gx (gx may be NULL, gx16 is ignored) -- the kernel computes gx = x W_ih^T + bias itself, slice by slice, from the 16-bit
     * operand images the projection GEMM would read, with that GEMM's summation and FT_GEMM_C16's rounding: y / gates / cell are
     * bit-identical to ft_gemm_img(FT_GEMM_C16) + gx16.  x_img: the compact row-mapped image of x (ft_bf16_image_rows over ft_rowmap_build
     * of `lens`: row of (t, b) = sum_{b' < b} (lens[b'] + 1) + t; x_rows rows of x_ld elements); the role must start at batch row 0 of that
     * map.  wih_img: the k-contiguous image of W_ih [4H][K] (ft_bf16_image; wih_ld elements per row).  x_bias: fp32 [4H] (b_ih + b_hh).
     * xproj_k = K: a multiple of 8, <= 128.  Images and bias 16-byte aligned, strides multiples of 8.  rows_per_group 4 or 8 only; one
     * projection mode per launch. */
    const void* x_img; const void* wih_img; const float* x_bias;
    int64_t x_ld, wih_ld, x_rows;
    int32_t xproj_k;
} ft_lstm_fwd_role;
typedef struct {
    const float* dy; int64_t ldy; const int32_t* lens; const float* gates; const float* cell;
    float* dgx;                          /* fp32 dgates rows [T][ldb][4H], or NULL when only the image is wanted */
    const void* wimg;
    void* dimg; int64_t dimg_ld; int64_t dimg_rows; float* dbias;    /* optional: as ft_lstm_persist_bwd_img (needs ldb == B) */
    float* state_da; float* state_dc;    /* [B][4H], [B][H] fp32: read when carry_in, written at the end of a non-empty window (zeros for rows
                                          * whose group has no step in it): the buffers need no initialisation */
    int32_t B, ldb, t0, t1, carry_in;    /* carry_in: the window [t1, ..) has run before and left its state */
} ft_lstm_bwd_role;
size_t ft_lstm_roles_ctx_bytes(void);
size_t ft_lstm_roles_wimg_bytes(int H);
int ft_lstm_roles_ctx_init(void* ctx, void* stream);
int ft_lstm_roles_debug_prof(void* dev_buf);        /* as ft_lstm_persist_debug_prof, for the kernels below */
int ft_lstm_roles_prepare_fwd(const float* w_hh, void* wimg, int H, void* stream);
int ft_lstm_roles_prepare_bwd(const float* w_hh, void* wimg, int H, void* stream);
/* The fragment images of up to 16 recurrent weights in ONE launch: each fp32 W_hh [4H][H] (contiguous, 16-byte aligned) is read once
 * and written as its forward image (fwd_img, what ft_lstm_roles_prepare_fwd makes) and / or its backward image (bwd_img, what
 * ft_lstm_roles_prepare_bwd makes -- also the image ft_lstm_persist_bwd builds for itself); a NULL destination is skipped, at least one
 * per weight is set.  Byte-identical to the per-weight entries. */
typedef struct { const float* w_hh; void* fwd_img; void* bwd_img; } ft_wfrag_desc;
int ft_lstm_roles_prepare_table(const ft_wfrag_desc* descs, int n, int H, void* stream);
int ft_lstm_roles_fwd(const ft_lstm_fwd_role* roles, int n_roles, int rows_per_group, int reset_rows, void* ctx, int phase,
                      int32_t* status, int H, void* stream);
int ft_lstm_roles_bwd(const ft_lstm_bwd_role* roles, int n_roles, int rows_per_group, int reset_rows, void* ctx, int phase,
                      int32_t* status, int H, void* stream);

/* Two stacked layers (the decoder nn.LSTM(.., num_layers=2), flowtron.py:654, :760-765) as ONE launch chain: layer 1 at
 * time t-1 and layer 0 at time t are two workgroup groups of the same launch, and layer 1's input projection
 * (h0 W_ih1^T) rides along as a second bf16 fragment stream, so T+1 launches replace 2T + a batched GEMM.
 * gx0 [T,B,4H] = x W_ih0^T + b0 (from ft_gemm), bias1 [4H] = b_ih1 + b_hh1; forward direction, bf16 MFMA operands.
 * Saves y/gates/cell of BOTH layers; backward returns dgx0 and dgx1 [T,B,4H] (weight/bias gradients follow as GEMMs /
 * column sums over all T*B rows: dW_hh0 = dgx0[1:]^T y0[:-1], dW_ih1 = dgx1^T y0, dW_hh1 = dgx1[1:]^T y1[:-1]).
 * Only for ft_lstm2_supported(B,H) (H % 128 == 0, B <= 64); work: ft_lstm2_workspace_bytes(B,H), 256-byte aligned. */
int ft_lstm2_supported(int B, int H);
size_t ft_lstm2_workspace_bytes(int B, int H);
int ft_lstm2_seq_fwd(const float* gx0, const float* w_hh0, const float* w_ih1, const float* bias1, const float* w_hh1,
                     const int32_t* lens, float* y0, float* gates0, float* cell0, float* y1, float* gates1, float* cell1,
                     void* work, int T, int B, int H, void* stream);
int ft_lstm2_seq_bwd(const float* dy1, const float* w_hh0, const float* w_ih1, const float* w_hh1, const int32_t* lens,
                     const float* gates0, const float* cell0, const float* gates1, const float* cell1,
                     float* dgx0, float* dgx1, void* work, int T, int B, int H, void* stream);

/* Both directions of a bidirectional layer (the encoder nn.LSTM(.., bidirectional=True), flowtron.py:488, :505-512) as ONE
 * launch chain: the forward-in-time and the reverse recurrence are independent and each step is latency-bound, so they run
 * as the two z-slices of the same launch (T launches instead of 2T).  bf16 MFMA operands; ft_lstm_bidir_supported(B,H):
 * H % 128 == 0, B <= 64.  y [T,B,ldy] with ldy >= 2H receives [h_fwd | h_rev]; dy has the same layout.  gx_*, gates_*,
 * cell_*, dgx_* as in ft_lstm_seq_*; work_f / work_r: ft_lstm_workspace_bytes(B,H) each, 256-byte aligned. */
int ft_lstm_bidir_supported(int B, int H);
int ft_lstm_bidir_seq_fwd(const float* gx_f, const float* gx_r, const float* w_hh_f, const float* w_hh_r,
                          const int32_t* lens, float* y, int64_t ldy, float* gates_f, float* gates_r,
                          float* cell_f, float* cell_r, void* work_f, void* work_r, int T, int B, int H, void* stream);
int ft_lstm_bidir_seq_bwd(const float* dy, int64_t ldy, const float* w_hh_f, const float* w_hh_r, const int32_t* lens,
                          const float* gates_f, const float* gates_r, const float* cell_f, const float* cell_r,
                          float* dgx_f, float* dgx_r, void* work_f, void* work_r, int T, int B, int H, void* stream);

/* Persistent form of ft_lstm_bidir_seq_* for the text encoder's shape (H == 256, B <= 32, 256-CU device, 16-bit operands): ONE launch
 * per pass for both directions and all time steps (csrc/bilstm_persist.hip: XCD-local hand-off; forward, every wave an independent
 * agent with no workgroup-level step; backward, K split over the four waves of a workgroup and summed in a fixed order).  Same
 * tensors as ft_lstm_bidir_seq_*; one workspace (ft_bilstm_persist_workspace_bytes, 256-byte aligned); `status` as for
 * ft_lstm_persist_*.  Same operand rounding as the launch-per-step chain, different fp32 summation order: results agree to
 * rounding, not bit for bit.  Deterministic; a row's results do not depend on the other rows of its batch. */
int ft_bilstm_persist_supported(int B, int H);
size_t ft_bilstm_persist_workspace_bytes(int B, int H);
/* debug: device buffer [1024][4][6] int64 that subsequent ft_bilstm_persist_bwd launches fill with the stage stamps (100 MHz wall
 * clock: step top, polled, partial written, reduced, cell done, published) of the four waves of one workgroup; NULL switches it off */
int ft_bilstm_persist_debug_prof(void* dev_buf);
int ft_bilstm_persist_fwd(const float* gx_f, const float* gx_r, const float* w_hh_f, const float* w_hh_r, const int32_t* lens,
                          float* y, int64_t ldy, float* gates_f, float* gates_r, float* cell_f, float* cell_r,
                          void* work, int32_t* status, int T, int B, int H, void* stream);
int ft_bilstm_persist_bwd(const float* dy, int64_t ldy, const float* w_hh_f, const float* w_hh_r, const int32_t* lens,
                          const float* gates_f, const float* gates_r, const float* cell_f, const float* cell_r,
                          float* dgx_f, float* dgx_r, void* work, int32_t* status, int T, int B, int H, void* stream);

/* ---- additive attention scores + softmax + prior posterior (flowtron.py:544-583)
 * Q [T,B,A] (time-major), K [L,B,A], v [A], in_lens [B], prior [B,T,L] or NULL.
 * e[b,t,l] = sum_a v[a] tanh(Q[t,b,a]+K[l,b,a]) / temperature, -inf at l >= in_lens[b];
 * p = softmax_l(e); with prior: logprob = log(p+1e-20)+log(prior+1e-20), attn = softmax_l(masked logprob);
 * without: attn = p, logprob = log(p+1e-8).  The B*T*L*A tanh tensor is never materialised.
 * Outputs attn, logprob [B,T,L]; p [B,T,L] is saved for backward when prior != NULL (may alias attn otherwise).
 * bwd: dattn, dlogprob (may be NULL) -> dQ [T,B,A], dK [L,B,A] (atomically accumulated: zero it first),
 * dv [A] (accumulated: zero it first). tanh is recomputed. */
int ft_attention_fwd(const float* Q, const float* K, const float* v, const int32_t* in_lens, const float* prior,
                     float* attn, float* logprob, float* p_save,
                     int T, int B, int L, int A, float temperature, void* stream);
int ft_attention_bwd(const float* Q, const float* K, const float* v, const int32_t* in_lens, const float* prior,
                     const float* attn, const float* p_save, const float* dattn, const float* dlogprob,
                     float* de_work, float* dQ, float* dK, float* dv,
                     int T, int B, int L, int A, float temperature, void* stream);

/* ---- affine coupling (flowtron.py:770-772) --------------------------------
 * out [T,B,2M] = [log_s | b];  z = exp(log_s)*x + b.
 * bwd: dout = [dz*x*exp(log_s) + dlog_s_ext | dz], dx = dz*exp(log_s)  (dlog_s_ext may be NULL). */
int ft_affine_fwd(const float* out, const float* x, float* z, int64_t n_rows, int M, void* stream);
int ft_affine_bwd(const float* out, const float* x, const float* dz, const float* dlog_s_ext,
                  float* dout, float* dx, int64_t n_rows, int M, void* stream);
/* inverse used by inference (flowtron.py:821): x = (z - b) / exp(log_s) */
int ft_affine_inv(const float* out, const float* z, float* x, int64_t n_rows, int M, void* stream);

/* ---- masked NLL partial sums (flowtron.py:206-235) -------------------------
 * acc[0] += sum_{t<len_b} z^2 ; acc[1] += sum_{t<len_b} log_s  (acc zeroed by caller).
 * x [T,B,M] with row stride ld (log_s is a strided view of the coupling output). */
int ft_masked_sum(const float* x, int64_t ld, const int32_t* lens, float* acc, int square,
                  int T, int B, int M, void* stream);
/* dx = scale_dev[0] * coef * (square ? x : 1) at valid positions, 0 at pads */
int ft_masked_sum_bwd(const float* x, int64_t ld, const int32_t* lens, const float* scale_dev, float coef, int square,
                      float* dx, int64_t ld_dx, int T, int B, int M, void* stream);

/* ---- gate BCE-with-logits (flowtron.py:237-243) ----------------------------
 * gate [T,B], target [B,T]; acc[0] += sum_valid BCE(gate, target).  bwd: dgate = scale*(sigmoid(g)-y) valid, 0 pads */
int ft_gate_bce_fwd(const float* gate, const float* target, const int32_t* lens, float* acc, int T, int B, void* stream);
int ft_gate_bce_bwd(const float* gate, const float* target, const int32_t* lens, const float* scale_dev, float coef,
                    float* dgate, int T, int B, void* stream);

/* ---- FlowtronLoss.forward's NLL + gate terms in four launches, their backward in two (flowtron.py:200-243; ABI 12) ------------
 * The per-term entry points above leave the scalar arithmetic (frame count, normalisers, g / n) to the caller -- ~40 four-byte
 * kernels per training step right where train.py:300-303 waits for the losses.  fwd: acc (8 floats, zeroed here) receives
 * [0] sum_valid z^2, [1] sum_f sum_valid log_s[f], [2] sum_valid BCE, and from a one-workgroup kernel [4] 1 / (n M), [5] 1 / n,
 * [6] n = sum_b min(max(out_lens[b], 0), T) -- the frames the masked sums visit (they mask with t < out_lens[b] over t < T, so a length
 * beyond T counts as T in n as well); nll_out[0] = (acc[0] / (2 sigma^2) - acc[1]) / (n M), gate_out[0] = acc[2] / n (gate, gate_target,
 * gate_out all NULL: no gate term).  z [T,B,M] contiguous; log_s = HOST array of n_ls (<= 8) device pointers to [T,B,M] views
 * with row stride ld_ls; gate [T,B], gate_target [B,T].
 * bwd (reads acc as fwd left it; g_nll / g_gate = device scalars, the gradients of the two outputs): dz = g_nll z / (sigma^2 n M),
 * dls = -g_nll / (n M) (ONE tensor: the gradient of every flow's log_s; may be NULL), dgate = g_gate (sigmoid(gate) - target) / n,
 * all zero at padded frames.  (g_nll, dz) and (g_gate, dgate) are each both NULL or both set. */
int ft_flowtron_loss_fwd(const float* z, const float* const* log_s, int n_ls, int64_t ld_ls, const float* gate,
                         const float* gate_target, const int32_t* out_lens, float sigma, float* acc, float* nll_out,
                         float* gate_out, int T, int B, int M, void* stream);
int ft_flowtron_loss_bwd(const float* z, const float* gate, const float* gate_target, const int32_t* out_lens, float sigma,
                         const float* acc, const float* g_nll, const float* g_gate, float* dz, float* dls, float* dgate,
                         int T, int B, int M, void* stream);

/* ---- reverse-by-length (flowtron.py:606-622, the flip+roll involution) --------
 * time_major=1: x,y [T,B,C]; time_major=0: x,y [B,T,C].
 * y[t] = x[len-1-t] (t < len), x[T-1+len-t] (t >= len). */
int ft_reverse_by_length(const float* x, float* y, const int32_t* lens, int T, int B, int C, int time_major, void* stream);

/* ---- activation backward (autograd of torch.tanh after nn.Linear, flowtron.py:461-464):
 * dpre = dy * act'(pre), written through the saved output y = act(pre).  dpre may alias dy. */
int ft_act_bwd(const float* y, const float* dy, float* dpre, int64_t n, int act, void* stream);

/* ---- elementwise out = a + b (op 0) or a * b (op 1): key modulation text*cond (flowtron.py:712) and the running
 * attention sum (:719) of the cumulative-attention branch.  out may alias a or b. */
int ft_eltwise(const float* a, const float* b, float* out, int64_t n, int op, void* stream);

/* ---- column sums (bias gradients): out[n] = sum_r x[r*ld + n] -------------- */
int ft_colsum(const float* x, float* out, int64_t rows, int N, int64_t ld, void* stream);

/* ---- autoregressive decode, batch 1 (flowtron.py:775-828) ------------------
 * One flow, N frames, fully enqueued without host synchronisation.  See ft_decode_args.
 * n_done_dev[0] receives the number of frames produced (gate stop, flowtron.py:823-826). */
typedef struct {
    /* attention_lstm */  const float *att_w_ih, *att_w_hh, *att_b_ih, *att_b_hh;
    /* attention     */   const float *w_query, *v, *K, *V;   /* K,V [L,A] precomputed once per utterance */
    /* lstm l0, l1   */   const float *l0_w_ih, *l0_w_hh, *l0_b_ih, *l0_b_hh, *l1_w_ih, *l1_w_hh, *l1_b_ih, *l1_b_hh;
    /* dense, conv   */   const float *d0_w, *d0_b, *d1_w, *d1_b, *conv_w, *conv_b;
    /* gate (or NULL)*/   const float *gate_w, *gate_b;
    const float* residual;   /* [N,M] */
    float* mel_out;          /* [N,M] */
    float* attn_out;         /* [N,L] */
    int32_t* n_done_dev;     /* [1] */
    void* work; size_t work_bytes;
    int N, L, H, A, M;
    float temperature, gate_threshold;
    int use_graph;
    /* cumulative / location-sensitive attention (flowtron.py:129-152, :793-806); all NULL when use_cumm_attention is off:
     * Conv1d(2->32,k5)+ReLU, Conv1d(32->E,k3)+Sigmoid over [cumulative attn ; previous attn]; the result scales the
     * encoder outputs enc [L,E] before the key projection w_key [A,E], every frame.  K is then ignored. */
    const float *cond_w1, *cond_b1, *cond_w2, *cond_b2, *w_key, *enc;
    int E;
    /* optional [N,L] rows: attention prior (attn = softmax(log(p+1e-20)+log(prior+1e-20)), flowtron.py:544-557, :799) and
     * forced alignment (the given row replaces the computed attention, :585-588, :798); NULL = off */
    const float *prior, *forced;
    /* optional scratch of ft_decode_wimg_bytes() bytes (256-byte aligned): when given, the ten weight matrices are rounded once
     * per call to bf16 images and the per-frame GEMVs stream those (bf16 operand mode: half the bytes per frame; fp32
     * activations and accumulation).  NULL = stream the fp32 weights (parity mode). */
    void* wimg; size_t wimg_bytes;
    /* optional: hand-off buffer of ft_decode_persist_gran_bytes() bytes + a device status word (zeroed by the caller once).  When
     * given together with wimg, and the flow has the default geometry (H 1024, A 640, M 80, L <= 1024, no cumulative attention /
     * prior / forced alignment) on a 256-CU device, the WHOLE flow runs as one persistent launch (256 workgroups hand each
     * stage's output vector to one another through tag-checked granules) instead of ten launches per frame.  *persist_status
     * becomes non-zero if a hand-off wait times out; the caller must check it before trusting the output. */
    void* persist_gran; int32_t* persist_status;
    /* decoder LSTM depth (ABI 11; nn.LSTM(n_hidden + n_attn, n_hidden, n_lstm_layers), flowtron.py:654-655): 0 or 2 = the two layers
     * above; 1 = layer 0 only (l1_* NULL); n > 2 = layers 2 .. n-1 from `extra_layers`, a HOST array of 4 (n - 2) device pointers
     * {w_ih [4H,H], w_hh [4H,H], b_ih, b_hh} per layer.  Depths other than 2 run on the staged chain (one launch per stage and
     * frame, hipGraph of 8 frames); layers beyond the second stream their fp32 weights in every operand mode. */
    int n_layers; const float* const* extra_layers;
} ft_decode_args;
size_t ft_decode_workspace_bytes(int L, int H, int A, int M, int E, int n_layers);
size_t ft_decode_wimg_bytes(int H, int A, int M);
size_t ft_decode_persist_gran_bytes(void);
int ft_decode_debug_prof(void* dev_buf);   /* debug: [512][12] int64 stage stamps of the persistent decode, NULL = off */
int ft_decode_flow(const ft_decode_args* a, void* stream);

/* ---- autoregressive decode of 2 .. ft_decode_batch_max() utterances of one flow in ONE persistent launch ------
 * Each utterance comes out bit for bit as ft_decode_flow's persistent launch decodes it alone: the hand-offs of a frame carry every
 * utterance still decoding.  `a` as for ft_decode_flow, with the per-utterance operands nb-strided: K, V [nb][L][A], residual,
 * mel_out [nb][N][M], attn_out [nb][N][L], n_done_dev [nb]; text is padded to the batch's L.  a.persist_gran (required) holds
 * ft_decode_batch_gran_bytes(nb) bytes, a.persist_status is required, a.wimg as for ft_decode_flow (NULL = fp32 weights);
 * wimg_ready != 0: a.wimg already holds the images of these weights (an earlier call of the same flow rounded them).  a.work and
 * a.use_graph are not used.  n_lim [nb] (device): frames of each utterance (<= N; gate stops end an utterance earlier).  Rows of
 * mel_out / attn_out past an utterance's end are not written.  FT_EINVAL: nb < 2 or > ft_decode_batch_max(), a NULL or misaligned
 * pointer (16 bytes; wimg 256).  FT_EUNSUPPORTED: outside the persistent geometry (H 1024, A 640, M 80, L <= 1024, two decoder
 * layers, no cumulative attention, prior or forced alignment) or not a 256-CU device.  Both before anything reaches the device.
 * ft_decode_flow_batch_keys: the same with a text length per utterance.  n_keys [nb] (device int32, each 1 ..= a.L; 4-byte
 * aligned): utterance b attends to key / value rows 0 .. n_keys[b]-1 of its K, V only, exactly as ft_decode_flow decodes it alone
 * at L = n_keys[b]; its attn_out columns >= n_keys[b] are not written (row stride stays a.L).  NULL = a.L for every utterance,
 * which is ft_decode_flow_batch.
 * ft_decode_flow_batch_forced: 1 .. ft_decode_batch_max() utterances ALONG GIVEN ALIGNMENT ROWS, in the same launch geometry (a
 * group of one included).  a.forced (required) is nb-strided like the other per-utterance operands: [nb][N][L] fp32, 16-byte
 * aligned, frame i of utterance b at forced[(b * N + i) * L], rows in the flow's own time order (a reversed flow's rows
 * reversed by the caller).  A frame takes its row as it is -- no scores, no softmax, no normalisation (what ft_decode_flow does
 * with a.forced) --, writes it verbatim to attn_out and multiplies it with V; columns >= n_keys[b] and rows >= n_lim[b] are never
 * read.  n_keys, n_lim, gate stops, wimg / wimg_ready, persist_gran and persist_status as above.  a.w_query and a.K may be NULL
 * (not read); a.temperature is accepted and unused.  With a.w_query NULL the query image slot of a.wimg is NOT written: a later
 * free-running call on the same a.wimg must round again (wimg_ready = 0), or it reads whatever the slot held.  FT_EUNSUPPORTED: nb < 1 or > ft_decode_batch_max(), a.forced NULL, a.prior
 * given, or outside the persistent geometry as above.  The result is the float arithmetic of the free-running launch on the given
 * rows, not that of ft_decode_flow's staged forced decode: the two sum in different orders. */
typedef struct {
    ft_decode_args a;
    int nb;
    const int32_t* n_lim;
    int wimg_ready;
} ft_decode_batch_args;
int ft_decode_batch_max(void);
size_t ft_decode_batch_gran_bytes(int nb);
int ft_decode_flow_batch(const ft_decode_batch_args* a, void* stream);
int ft_decode_flow_batch_keys(const ft_decode_batch_args* a, const int32_t* n_keys, void* stream);
int ft_decode_flow_batch_forced(const ft_decode_batch_args* a, const int32_t* n_keys, void* stream);

/* ---- STFT magnitude + mel + log (audio_processing.py:117-134, 207-235) -------
 * y [B,N] in [-1,1] -> mel [B,n_mel,N/hop+1]; window [n_fft] (periodic hann),
 * fb [n_mel, n_fft/2+1].  Radix-2 real FFT per frame in LDS (n_fft = 1024). */
int ft_stft_mel(const float* y, const float* window, const float* fb, float* mel,
                int B, int N, int n_fft, int hop, int n_mel, void* stream);
/* The same front end for the reference's analysis setting n_fft = 1024, hop <= 256 (config.json:32-34) as a REAL FFT (one
 * 512-point complex FFT + split step, one wave per frame, radix-8 passes in registers) with the triangular filterbank in
 * sparse form: band b = weights band_w[band_ptr[b] .. band_ptr[b+1]) over the consecutive bins starting at band_bin0[b].
 * Any of mel [B,n_mel,T], (mag, phase) [B,513,T] may be requested (NULL = skip; mag and phase together = STFT.transform,
 * audio_processing.py:207-235).  window: hann [1024] (win_length zero-padded by the caller). */
int ft_stft_r8(const float* y, const float* window, const int32_t* band_bin0, const int32_t* band_ptr, const float* band_w,
               float* mel, float* mag, float* phase, int B, int N, int hop, int n_mel, void* stream);
/* The collated batch of the data path (data.py:149-155 per item, :207-229 zero padding) in ONE launch:
 * y [B,N] zero-padded audio, utterance b holds n_samples[b] samples (device int32) -> mel [B,n_mel,T_out]: the frames
 * t < n_samples[b] / hop + 1 exactly as ft_stft_r8 computes them for that utterance alone (reflect padding about ITS last
 * sample), zeros beyond -- the tensor DataCollate builds on the host.  T_out >= max_b (n_samples[b] / hop + 1). */
int ft_stft_r8_ragged(const float* y, const int32_t* n_samples, const float* window, const int32_t* band_bin0,
                      const int32_t* band_ptr, const float* band_w, float* mel, int B, int N, int hop, int n_mel, int T_out,
                      void* stream);
/* Inverse STFT (audio_processing.py:237-263, STFT.inverse) for the same setting n_fft = 1024, hop <= 256: (mag, phase) [B,513,T]
 * -> y [B, hop (T-1)] = the windowed irfft of every frame M e^{i phase} (Im of bins 0 and 512 ignored), overlap-added, divided by
 * the window's sum-square envelope where that is > FLT_MIN, first and last 512 samples cut.  Deterministic: no atomics, each
 * sample sums its frames in ascending t.  window: hann [1024] as ft_stft_r8.  T >= 2. */
int ft_istft_r8(const float* mag, const float* phase, const float* window, float* y, int B, int T, int hop, void* stream);
/* The synthesis side of a ragged batch (griffin_lim_ragged), ONE launch per batch each, on the kernels of the dense forms:
 * ft_stft_r8_ragged_phase: y [B,N], utterance b holds n_samples[b] samples (device int32) -> mag (NULL = the magnitude store is
 * skipped) and phase [B,513,N/hop+1]: frames t < n_samples[b] / hop + 1 exactly as ft_stft_r8 computes them for
 * y[b, :n_samples[b]] alone (reflect padding about ITS last sample; later samples are never read), zeros beyond in every
 * output that is written.
 * ft_istft_r8_ragged: (mag, phase) [B,513,T] with row stride T, utterance b holds n_frames[b] frames (device int32,
 * 1 <= n_frames[b] <= T) -> y [B, hop (T-1)]: samples n < hop (n_frames[b] - 1) exactly as ft_istft_r8 computes them for
 * mag[b, :, :n_frames[b]] alone (covering frames, wss and both trims from ITS frame count), zeros behind; frames
 * t >= n_frames[b] are never read.  No atomics, launch-independent.  Preconditions as the dense forms. */
int ft_stft_r8_ragged_phase(const float* y, const int32_t* n_samples, const float* window, float* mag, float* phase, int B, int N,
                            int hop, void* stream);
int ft_istft_r8_ragged(const float* mag, const float* phase, const int32_t* n_frames, const float* window, float* y, int B, int T,
                       int hop, void* stream);
/* The same three for every power-of-two analysis size n_fft = 256 .. 4096 and any hop (csrc/stft_pow2.hip): an n_fft/2-point
 * complex FFT (Stockham, one radix-2 / -4 pass and radix-8 passes, one wave per frame) plus the split step.  Bins: n_fft/2+1.
 * 1 <= hop <= win_length <= n_fft; window: hann [n_fft] (win_length zero-padded by the caller); N > n_fft / 2.  Outputs, the
 * ragged form and the inverse's rules (ascending-t overlap-add, wss in the kernel, > FLT_MIN, both n_fft/2 trims) as above.
 * Arguments outside that scope: FT_EINVAL before any device call. */
int ft_stft_pow2(const float* y, const float* window, const int32_t* band_bin0, const int32_t* band_ptr, const float* band_w,
                 float* mel, float* mag, float* phase, int B, int N, int n_fft, int hop, int win_length, int n_mel, void* stream);
int ft_stft_pow2_ragged(const float* y, const int32_t* n_samples, const float* window, const int32_t* band_bin0,
                        const int32_t* band_ptr, const float* band_w, float* mel, int B, int N, int n_fft, int hop, int win_length,
                        int n_mel, int T_out, void* stream);
int ft_istft_pow2(const float* mag, const float* phase, const float* window, float* y, int B, int T, int n_fft, int hop,
                  int win_length, void* stream);
/* ft_stft_r8_ragged_phase / ft_istft_r8_ragged for the power-of-two sizes: the same contracts against ft_stft_pow2 /
 * ft_istft_pow2, bins n_fft/2+1, trims n_fft/2. */
int ft_stft_pow2_ragged_phase(const float* y, const int32_t* n_samples, const float* window, float* mag, float* phase, int B,
                              int N, int n_fft, int hop, int win_length, void* stream);
int ft_istft_pow2_ragged(const float* mag, const float* phase, const int32_t* n_frames, const float* window, float* y, int B,
                         int T, int n_fft, int hop, int win_length, void* stream);

/* ---- sample-rate conversion (csrc/resample.hip; additive, not in the reference) ----------------------
 * x [B,N] at `orig` Hz -> y [B,N_out] at `new` Hz by the Hann-windowed sinc of width W = 6 zero crossings and rolloff 0.99:
 *   y[m] = sum_{0 <= k < n} h(k / orig - m / new) x[k],   base = 0.99 min(orig, new),
 *   h(t) = (base / orig) sinc(base t) cos^2(pi base t / (2 W)) for |base t| < W, else 0.
 * With g = gcd(orig, new), orig_g = orig / g, new_g = new / g: output m = q new_g + p sums, in ascending k, the K inputs
 * k = q orig_g + phase_start[p] + i against taps[p][i] (both built by the caller, device buffers: taps fp32 [new_g][K],
 * phase_start int32 [new_g], non-decreasing in p with phase_start[new_g-1] <= phase_start[0] + orig_g).
 * Utterance b holds n_samples[b] samples (device int32, 1 ..= N; NULL = N each): y[b, m] for m < ft_resample_out_len(
 * n_samples[b], orig, new) exactly as the utterance resampled alone, zeros behind up to N_out; samples behind n_samples[b]
 * are never read.  One launch, no atomics.  FT_EUNSUPPORTED when the table exceeds FT_RESAMPLE_MAX_PHASES phases or
 * FT_RESAMPLE_MAX_TAPS taps in all (every ordered pair of 8 / 11.025 / 16 / 22.05 / 24 / 32 / 44.1 / 48 kHz fits). */
#define FT_RESAMPLE_MAX_PHASES 2048
#define FT_RESAMPLE_MAX_TAPS 20480
int ft_resample_ragged(const float* x, const int32_t* n_samples, const float* taps, const int32_t* phase_start, float* y,
                       int B, int N, int N_out, int orig_g, int new_g, int K, void* stream);
/* host arithmetic only: ceil(n new / orig) in 64 bits; -1 for n < 0 or a rate < 1 */
int64_t ft_resample_out_len(int64_t n, int orig, int new_rate);

/* ---- style transfer: posterior over z from reference utterances (inference_style_transfer.ipynb; csrc/style.hip) -------
 * The notebook's posterior mean of z given K reference latents z_b [M][len_b] under the prior N(0, 1):
 *   ratio = K / lambd,   mu = ratio / (ratio + 1) * acc / K,   acc summed over the utterances b:
 *   FT_STYLE_BATCH           acc [M][n_frames]:  acc[m][t] += z_b[m][t mod len_b]   (every utterance tiled along time)
 *   FT_STYLE_TIME_AND_BATCH  acc [M]:            acc[m] += (sum_{t < len_b} z_b[m][t]) / len_b   (n_frames is not used: pass 1)
 * accumulate: adds the B utterances of one batch, in order of b, into the float64 accumulator `acc`, which the caller owns
 * and zeroes once per reference set.  z is fp32 with ELEMENT strides (utterance, mel, frame), so the forward's time-major
 * [T][B][M] output and a [B][M][T] tensor are both read in place; lens [B] device int32, clamped to 1 ..= T inside the
 * kernel; frames at or behind lens[b] are never read.  One launch, no floating-point atomics: each element of acc belongs
 * to one thread, a time sum is 16 strided partial sums (t = j, j + 16, ..., ascending) folded by one fixed tree.  A reference
 * set therefore gives the same bits however it is split into calls and whatever T its batches are padded to.
 * sample: out [S][M][n_frames] fp32 = mu + sigma * eps[s][m][t] (TIME_AND_BATCH: mu[m] at every t), formed in float64 and
 * rounded to fp32 once; eps fp32 [S][M][n_frames] standard normal draws of the caller's, or NULL with S = 1: out = mu.
 * K = the utterances accumulated so far.  One launch.
 * FT_EINVAL before any device call: a NULL pointer (but eps), B, M, T, n_frames, S or K < 1, lambd <= 0, a negative stride,
 * an unknown mode, eps == NULL with S != 1, acc not 8-byte aligned, M > 16 * 65535 (the accumulate grid). */
enum { FT_STYLE_BATCH = 0, FT_STYLE_TIME_AND_BATCH = 1 };
int ft_style_accumulate(const float* z, int64_t stride_b, int64_t stride_m, int64_t stride_t, const int32_t* lens, double* acc,
                        int B, int M, int T, int n_frames, int mode, void* stream);
int ft_style_sample(const double* acc, const float* eps, float* out, int S, int M, int n_frames, int K, double lambd,
                    double sigma, int mode, void* stream);

/* ---- token durations and alignments from durations (csrc/align.hip; additive, not in the reference) -------------------
 * mas_ragged: monotonic alignment search over a ragged batch, one launch, one workgroup per utterance.  logp: fp32 scores
 * with ELEMENT strides (utterance, frame, token), so a slice of the forward's attn_logprob [B][T][L] or of a stacked
 * [F][B][T][L] tensor is read in place; in_lens / out_lens [B] device int32, clamped inside the kernel to 1 ..= L and 1 ..= T;
 * only scores with t < T_b = out_lens[b] and l < L_b = in_lens[b] are read.  Per utterance
 *     Q[0][0] = s[0][0];   Q[t][l] = s[t][l] + (adv[t][l] ? Q[t-1][l-1] : Q[t-1][l])   for l <= min(t, L_b - 1)
 *     adv[t][l] = l > 0 && (l == t || Q[t-1][l-1] > Q[t-1][l])     (strict: a tie stays)
 *     backtrack from (T_b - 1, L_b - 1):  path[t] = l;  l -= adv[t][l]
 * one fp32 add and one compare per cell, so a float32 replay on the host gives the same bits.  Among the best-scoring
 * monotone paths this is the one that advances earliest, and it is structurally valid whatever the scores (all -inf too):
 * path[0] = 0, path[T_b-1] = L_b - 1, steps of 0 or 1.
 * path [B][T] int32, -1 behind T_b; durations [B][L] int32: frames per token, each >= 1, sum T_b, 0 behind L_b; score [B] fp32
 * = Q[T_b-1][L_b-1], or NULL.  An utterance with L_b > T_b has no monotone path: path -1, durations 0, score -inf.
 * work: the backpointers, one bit per cell, mas_workspace_bytes bytes (host arithmetic only; 0 for a size < 1), 8-byte
 * aligned; contents need not be initialised.  No atomics, no communication between workgroups.
 * durations_to_rows: rows [B][N][L] fp32, rows[b][n][l] = 1 where cum[l-1] <= n < cum[l] and l < in_lens[b], with cum the
 * running sum of max(durations[b][l], 0); every other element 0, rows at or behind the utterance's total included.
 * reverse != 0: utterance b's rows in reversed time (row n holds frame total_b - 1 - n), the order an odd flow decodes in.
 * One launch; the scan over L runs inside each workgroup.
 * FT_EINVAL before any device call: a NULL pointer (but score), B, T, L or N < 1, a negative stride, work misaligned or
 * work_bytes too small.  FT_EUNSUPPORTED: mas_ragged with L > 1024 (the text limit of the batched decode). */
size_t ft_mas_workspace_bytes(int B, int T, int L);
int ft_mas_ragged(const float* logp, int64_t stride_b, int64_t stride_t, int64_t stride_l, const int32_t* in_lens,
                  const int32_t* out_lens, int32_t* path, int32_t* durations, float* score, void* work, size_t work_bytes,
                  int B, int T, int L, void* stream);
int ft_durations_to_rows(const int32_t* durations, const int32_t* in_lens, float* rows, int B, int N, int L, int reverse,
                         void* stream);

/* ---- mel-cepstral distortion along a dynamic-time-warping path (csrc/dtw.hip; additive, not in the reference) ----------
 * mel_cepstra: truncated cepstra of log-mel frames.  mel: fp32 with ELEMENT strides (utterance, mel channel, frame), so a
 * [B][M][T] tensor or any view of one is read in place; lens [B] device int32, clamped inside the kernel to 1 ..= T, or NULL
 * for T frames everywhere; dct [K][M] fp32, row k-1 the DCT-II basis sqrt(2/M) cos(pi k (m + 0.5) / M) that the caller
 * builds in float64 and rounds once (c0 is left out); cep [B][T][K] fp32 contiguous:
 *     cep[b][t][k-1] = sum_m mel[b][m][t] * dct[k-1][m]        m ascending, every product and every sum rounded on its own
 * Frames at or behind lens[b] are not read and their outputs are not written.  One launch.
 * dtw_ragged: one pair of feature sequences per utterance, one launch, one workgroup per pair.  x [B][Ta][K] and y [B][Tb][K]
 * fp32 with ELEMENT strides (pair, frame, feature); x_lens / y_lens [B] device int32, clamped inside the kernel to 1 ..= Ta
 * and 1 ..= Tb; nothing at or behind A = x_lens[b] and N = y_lens[b] is read.  Per pair, every operation an fp32 operation
 * rounded once (nothing is contracted into a fused multiply-add, the square root is correctly rounded):
 *     d[i][j] = sqrt(sum_k (x[i][k] - y[j][k])^2)              k ascending
 *     C[0][0] = d[0][0];   i == 0: move 2, from (i, j-1);   j == 0: move 1, from (i-1, j)
 *     else  best = C[i-1][j-1], move 0;  if C[i-1][j] < best: best, move 1;  if C[i][j-1] < best: best, move 2
 *     C[i][j] = d[i][j] + best;   backtrack from (A-1, N-1) to (0, 0)
 * so a float32 replay on the host gives the same bits.  The compares are strict: a tie keeps the earlier move (diagonal
 * before up before left; x and y are therefore NOT interchangeable), and the border moves do not look at the costs, so the
 * path is structurally valid whatever the features hold (NaN and inf too).
 * cost [B] fp32 = C[A-1][N-1]; path_len [B] int32; path [B][Ta + Tb - 1][2] int32: the cells (i, j) in ascending order, -1
 * behind path_len[b].  diagonal != 0: only the cells i == j, cost = the running sum of d[i][i] over ascending i, path_len A;
 * a pair with A != N has no such path: path_len 0, cost +inf, path -1.
 * work: the backpointers, two bits per cell, dtw_workspace_bytes bytes (host arithmetic only; 0 for a size < 1), 16-byte
 * aligned; contents need not be initialised.  No atomics, no communication between workgroups.
 * FT_EINVAL before any device call: a NULL pointer (but lens of mel_cepstra), B, M, T, Ta, Tb or K < 1, a negative stride,
 * B > 65535 (mel_cepstra), work misaligned or work_bytes too small.  FT_EUNSUPPORTED: mel_cepstra with K > 32, K >= M or
 * M > 128; dtw_ragged with Ta or Tb > 1024 (a thread per column of y, the rows of x in LDS) or K > 32. */
int ft_mel_cepstra(const float* mel, int64_t stride_b, int64_t stride_m, int64_t stride_t, const int32_t* lens, const float* dct,
                   float* cep, int B, int M, int T, int K, void* stream);
size_t ft_dtw_workspace_bytes(int B, int Ta, int Tb, int K);
int ft_dtw_ragged(const float* x, int64_t x_stride_b, int64_t x_stride_t, int64_t x_stride_k, const float* y, int64_t y_stride_b,
                  int64_t y_stride_t, int64_t y_stride_k, const int32_t* x_lens, const int32_t* y_lens, float* cost,
                  int32_t* path_len, int32_t* path, void* work, size_t work_bytes, int B, int Ta, int Tb, int K, int diagonal,
                  void* stream);

/* ---- F0 tracking (YIN) and F0 error along a warping path (csrc/pitch.hip; additive, not in the reference; functions added
 * at ABI 15) ----------
 * f0_yin_ragged: one launch for a zero-padded batch.  audio: fp32 with ELEMENT strides (utterance, sample), so a [B][N]
 * tensor or any view of one is read in place; n_samples [B] device int32, clamped inside the kernel to 1 ..= N; f0 and
 * aperiodicity [B][T] fp32 contiguous, T = N / hop + 1.  Utterance b has T_b = n_samples[b] / hop + 1 frames; frame t reads
 * x[t hop - W/2 + j] for 0 <= j < W + tau_max + 1, samples before 0 or at or behind n_samples[b] read as 0 and their memory
 * is never touched; outputs at t >= T_b are 0.  Per frame, every operation an fp32 operation rounded once (nothing is
 * contracted into a fused multiply-add, the divisions are correctly rounded), so a float32 replay on the host gives the same
 * bits:
 *     d(tau) = sum_{j < W} (x[j] - x[j + tau])^2               tau = 0 .. tau_max + 1; j ascending: difference, square, add
 *     s(tau) = s(tau - 1) + d(tau), ascending from s(0) = 0
 *     d'(0) = 1;  d'(tau) = (d(tau) * float(tau)) / s(tau) where s(tau) > 0, and 1 where it is not (digital silence)
 *     tau = the lowest lag in tau_min ..= tau_max with d'(tau) < threshold; from there upwards while tau < tau_max and
 *           d'(tau + 1) < d'(tau)
 *     voiced (such a lag exists): a, b, c = d'(tau - 1), d'(tau), d'(tau + 1), den = (a + c) - 2 b,
 *           shift = (0.5 (a - c)) / den when a >= b, c >= b and den > 0, else 0;
 *           f0 = sampling_rate / (float(tau) + shift), aperiodicity = b
 *     unvoiced: f0 = 0, aperiodicity = the least d' in tau_min ..= tau_max
 * A frame whose window holds a non-finite sample gives f0 = 0 (its aperiodicity is unspecified); other frames are untouched.
 * f0_path_stats: per pair b over the cells c < path_len[b] of path [B][P][2] (int32 (i, j), as dtw_ragged writes them):
 * n_both [B] int32 = cells with f0_a[i] > 0 and f0_b[j] > 0, n_mismatch [B] int32 = cells where exactly one is, sum_sq [B]
 * float64 = the sum over the former of (1200 log2(f0_a[i] / f0_b[j]))^2, float64 throughout.  f0_a [B][Ta], f0_b [B][Tb]
 * fp32 with ELEMENT strides (pair, frame).  One launch, one workgroup per pair, a fixed order of summation: the same bits on
 * every call.  path_len is clamped to 0 ..= P and every index to its tensor inside the kernel, so a bad path reads nothing
 * out of bounds.  No atomics.
 * FT_EINVAL before any device call: a NULL pointer, B, N, hop, W, Ta, Tb or P < 1, a negative stride, B > 65535 or
 * sampling_rate <= 0 (f0_yin_ragged), tau_min < 2, tau_max < tau_min, a threshold outside (0, 1], P > Ta + Tb - 1 (a
 * monotone path has no more cells: a longer one leaves the tensors).  FT_EUNSUPPORTED: f0_yin_ragged with W > 2048, odd W
 * or tau_max > 1022. */
int ft_f0_yin_ragged(const float* audio, int64_t stride_b, int64_t stride_n, const int32_t* n_samples, float* f0,
                     float* aperiodicity, int B, int N, float sampling_rate, int hop, int W, int tau_min, int tau_max,
                     float threshold, void* stream);
int ft_f0_path_stats(const float* f0_a, int64_t a_stride_b, int64_t a_stride_t, const float* f0_b, int64_t b_stride_b,
                     int64_t b_stride_t, const int32_t* path, const int32_t* path_len, int32_t* n_both, int32_t* n_mismatch,
                     double* sum_sq, int B, int Ta, int Tb, int P, void* stream);

/* ---- F0 through noise: probabilistic YIN (Mauch & Dixon, "pYIN", ICASSP 2014; csrc/pitch.hip; additive, not in the
 * reference; functions added at ABI 15, no layout changes) ----------
 * Two launches with no host work between them: f0_candidates_ragged gives every frame a distribution over pitch bins,
 * f0_viterbi_ragged takes one path through a voiced / unvoiced pitch HMM.  audio, strides, n_samples, frames, N, hop, W, tau_min
 * and tau_max are f0_yin_ragged's, and d, s and d' are formed by the same code: the same bits.  Every arithmetic step below is
 * one fp32 operation rounded once, nothing is contracted, divisions are correctly rounded, comparisons are plain (a NaN makes
 * none true), so a float32 replay on the host gives the same bits; the tables are made on the host in float64 and rounded once.
 * f0_candidates_ragged.  Tables: cum [101] fp32, cum[i] = the Beta(a, b) distribution function at i / 100 (cum[0] = 0,
 * cum[100] = 1): the prior weight of the thresholds float(1) / 100 .. float(i) / 100; lag_edges [n_bins + 1] fp32, DESCENDING:
 * bin k holds the lags L with lag_edges[k + 1] < L <= lag_edges[k] (lag_edges[i] = sampling_rate / (fmin 2^((i - 1/2) / (12
 * bins_per_semitone))) where bin k is centred on fmin 2^(k / (12 bins_per_semitone)); the kernel takes no logarithm).
 * With n(v) = how many i in 1 .. 100 have float(i) / 100.f <= v  (n(+inf) = 100), per frame:
 *     trough:     a lag tau in tau_min ..= tau_max with d'(tau) <= d'(tau - 1) and d'(tau) < d'(tau + 1)
 *     candidate:  walking the troughs upwards with rec = +inf, a trough with d'(tau) < rec; its weight is
 *                 w = cum[n(rec)] - cum[n(d'(tau))]  (the thresholds it is the first trough below), then rec = d'(tau)
 *     global minimum: least = +inf, lags ascending, d'(tau) < least takes over (the lowest lag of equals; none if no d' is below
 *                 +inf); its weight is w = absolute_min_prob * cum[n(least)]
 *     an entry's lag is L = float(tau) + shift with f0_yin_ragged's parabolic shift, its frequency sampling_rate / L, its bin
 *                 the one that holds L; entries with w <= 0 or L outside the bins are dropped
 *     prob[k] = the sum of w over the entries of bin k, from 0, candidates in ascending lag order, the global minimum last;
 *     freq[k] = the frequency of its heaviest entry (the earliest of equals), 0 for a bin without entries
 *     voiced_prob = sum of prob: p[l] = prob[l] + prob[l + 64] + .. ascending from 0 for l = 0 .. 63, then for h = 32, 16, .. 1:
 *                 p[l] = p[l] + p[l + h] for l < h; the result is p[0]
 * A frame whose window holds a non-finite sample, a frame with s(tau_max + 1) = 0 (digital silence: s is ascending) and the
 * frames at t >= T_b have prob = freq = voiced_prob = 0.  prob, freq [B][T][n_bins], voiced_prob [B][T] fp32 contiguous.
 * f0_viterbi_ragged.  States (bin k, x), x = 1 voiced, x = 0 unvoiced; state number j = 2 k + x.  Tables: transition
 * [2 band + 1] fp32, transition[o] = (band + 1 - |o - band|) / (band + 1)^2, the weight of coming from bin k + o - band (bins
 * outside 0 .. n_bins - 1 have score 0; rows at the edges are not renormalised); centres [n_bins] fp32 Hz.  stay = 1.f -
 * switch_prob.  Per frame t of an utterance, with FLOOR = 2^-20 and CUT = 2^-64:
 *     obs(k, 1) = max(prob[t][k], FLOOR);   obs(k, 0) = max(max(1.f - voiced_prob[t], 0) / float(n_bins), FLOOR)
 *     t = 0:  r_0(k, x) = obs(k, x)                                             (the uniform start is a common factor: left out)
 *     t > 0:  A(k, x) = max over o = 0 .. 2 band of r_{t-1}(k + o - band, x) * transition[o]; the lowest o of equals
 *             keep = A(k, x) * stay;  change = A(k, 1 - x) * switch_prob;  the predecessor changes voicing when change > keep
 *             r_t(k, x) = ((the larger) * scale_{t-1}) * obs(k, x), and 0 where that is below CUT
 *     scale_t = the power of two 2^-e with 2^e <= max r_t < 2^(e + 1): exact, so no logarithm is taken anywhere
 * FLOOR keeps a frame from killing every path; CUT and 2^-20 <= switch_prob <= 1 - 2^-20 keep every product a normal number,
 * so the rule does not lean on how denormals are treated.  The path ends in the state with the largest r at the last frame,
 * the lowest j of equals, and goes back along the recorded predecessors.  f0[t] = 0 for an unvoiced state, else freq[t][k] if
 * that is > 0, else centres[k]; f0 is 0 at t >= T_b.  An utterance's result does not depend on its batch.
 * work: one byte per (frame, state): (o << 1) | voicing of the predecessor; f0_viterbi_workspace_bytes bytes (host arithmetic
 * only; 0 for a size < 1); contents need not be initialised.  One workgroup per utterance, one lane per state, one barrier
 * per frame.  No atomics, no scratch, no communication between workgroups in either kernel.
 * FT_EINVAL before any device call: a NULL pointer, B, N, hop, W or n_bins < 1, band < 0, a negative stride, B > 65535,
 * sampling_rate <= 0, tau_min < 2, tau_max < tau_min, absolute_min_prob outside [0, 1], switch_prob outside [2^-20, 1 - 2^-20],
 * work_bytes too small.  FT_EUNSUPPORTED: W > 2048, odd W, tau_max > 1022, n_bins > 512 (a lane per state), band > 63 (a byte
 * per backpointer). */
int ft_f0_candidates_ragged(const float* audio, int64_t stride_b, int64_t stride_n, const int32_t* n_samples, const float* cum,
                            const float* lag_edges, float* prob, float* freq, float* voiced_prob, int B, int N,
                            float sampling_rate, int hop, int W, int tau_min, int tau_max, int n_bins, float absolute_min_prob,
                            void* stream);
size_t ft_f0_viterbi_workspace_bytes(int B, int T, int n_bins);
int ft_f0_viterbi_ragged(const float* prob, const float* freq, const float* voiced_prob, const int32_t* n_samples,
                         const float* transition, const float* centres, float* f0, void* work, size_t work_bytes, int B, int N,
                         int hop, int n_bins, int band, float switch_prob, void* stream);

/* ---- mel -> waveform: NNLS mel inversion and the fast Griffin-Lim momentum step (csrc/vocode.hip; additive, not in the
 * reference; functions added at ABI 15) ----------
 * mel_nnls: one launch; per frame t of utterance b, min ||W m - s||^2 over m >= 0 by n_iters (>= 0) Lee-Seung multiplicative
 * updates.  s [B][n_mel][T] the linear mel, m0 [B][nb][T] the starting estimate, m [B][nb][T] the result (m may be m0), all
 * fp32 contiguous, nb = n_fft / 2 + 1.  n_frames [B] device int32, clamped inside the kernel to 0 ..= T, or NULL for T frames
 * everywhere: frames at or behind n_frames[b] are never read (neither s nor m0) and m holds 0 there.
 * W [n_mel][nb] comes twice.  By band, as TacotronSTFT's CSR: band j covers the len_j = fb_ptr[j+1] - fb_ptr[j] consecutive bins
 * from fb_bin0[j] with the weights fb_w[fb_ptr[j] ..], nnz = fb_ptr[n_mel] weights in all.  By bin: bin_band [nb][2] int32 the
 * bands that cover bin k, lower band first, -1 = none (a covered bin has [0] >= 0), bin_w [nb][2] fp32 their weights; a bin may
 * lie in at most two bands.  Per frame, every operation an fp32 operation rounded once (nothing is contracted into a fused
 * multiply-add, the divisions are correctly rounded), so a float32 replay on the host gives the same bits:
 *     band(x)[j] = sum_{i < len_j} fb_w[fb_ptr[j] + i] * x[fb_bin0[j] + i]        from 0, i ascending: product, then add
 *     bin(y)[k]  = bin_w[k][0] * y[bin_band[k][0]]  ( + bin_w[k][1] * y[bin_band[k][1]] when bin_band[k][1] >= 0 )
 *     start: p[l] = sum of m0[k] over k = l, l + 16, l + 32, ... ascending from 0 (l = 0 .. 15); mean = (p[0] + ... + p[15],
 *            ascending from 0) / float(nb); low = 1e-3f * mean;  m[k] = (m0[k] < low ? low : m0[k]) on covered bins, 0 elsewhere
 *     q = bin(s) once;   each iteration:  r = band(m);  d = bin(r);  m[k] = d[k] > 0 ? (m[k] * q[k]) / d[k] : 0 on covered bins,
 *            then m[k] = 0 where m[k] < 1e-30f (so the rule does not lean on how denormals are treated)
 * An all-zero frame gives zeros; n_iters = 0 returns the start.  Band ranges and band numbers are clamped to their arrays inside
 * the kernel.  No atomics, no scratch, no communication between workgroups.
 * gl_momentum: one elementwise launch over [B][n_bins][T] between the analysis and the synthesis launch of a Griffin-Lim
 * iteration: with c = magnitude * (cos(phase), sin(phase)) (sincosf; the transform's own magnitude and phase),
 *     first == 0:  t = c + alpha * (c - c_prev) per component (difference, product, add);  phase = atan2f(t.im, t.re)
 *     first != 0:  phase stays as it is (it is not written)
 *     always:      c_prev = c                  (prev_re, prev_im: two fp32 planes of the same shape, read only when first == 0)
 * n_frames as above (or NULL): cells at or behind n_frames[b] are neither read nor written.
 * FT_EINVAL before any device call: a NULL pointer (but n_frames), B, n_mel, T, nnz or n_bins < 1, n_iters < 0, B > 65535,
 * n_bins * T beyond 2^31 - 257, alpha outside [0, 1).  FT_EUNSUPPORTED: mel_nnls with n_fft not a power of two in 256 .. 4096,
 * n_mel > 128, or more weights than the workgroup's LDS holds beside one frame. */
int ft_mel_nnls(const float* s, const float* m0, float* m, const int32_t* n_frames, const int32_t* fb_bin0, const int32_t* fb_ptr,
                const float* fb_w, const int32_t* bin_band, const float* bin_w, int B, int n_mel, int n_fft, int T, int nnz,
                int n_iters, void* stream);
int ft_gl_momentum(const float* magnitude, float* phase, float* prev_re, float* prev_im, const int32_t* n_frames, int B, int n_bins,
                   int T, float alpha, int first, void* stream);

/* ---- mel -> waveform: the single-pass phase start of Griffin-Lim (SPSI: Beauregard, Harish, Wyse, "Single Pass Spectrogram
 * Inversion", DSP 2015; csrc/vocode.hip; additive, not in the reference; a function added at ABI 15, no layout changes) ----------
 * spsi_phase: one launch for the batch, one workgroup per utterance.  magnitude, phase [B][K][T] fp32 contiguous as the STFT
 * kernels write them, K = n_fft / 2 + 1.  n_frames [B] device int32, clamped inside the kernel to 0 ..= T, or NULL for T frames
 * everywhere: cells at or behind n_frames[b] hold 0 and their magnitudes are never read.
 * The phase is kept in TURNS (cycles): a wrap is a subtraction of rintf (round half to even), and hundreds of frames of hop
 * samples do not eat the mantissa.  Per utterance the frames t = 0, 1, .. are walked in order with an accumulator acc[K], all
 * zeros before frame 0.  Every operation an fp32 operation rounded once (nothing is contracted into a fused multiply-add, the
 * division is correctly rounded), the comparisons plain (a NaN makes none true), so a float32 replay on the host gives the
 * same bits.  With m[k] = magnitude[b][k][t]:
 *     peak:   bin k is a peak when 1 <= k <= K - 2, m[k] > m[k-1] and m[k] > m[k+1]
 *     offset: a, b, c = m[k-1], m[k], m[k+1];  den = (a - b) + (c - b);  p = (0.5f * (a - c)) / den;  p = 0 unless |p| <= 0.5f
 *             (that covers den = 0, inf and NaN)
 *     inc[k] = float((hop * k) mod n_fft) / float(n_fft) + (float(hop) / float(n_fft)) * p       (turns; the whole turns of
 *             hop * k / n_fft are taken out in integer arithmetic; quotient, quotient, product, sum)
 *     owner of bin j: a peak owns itself.  Otherwise, if j < K - 1 and m[j] < m[j+1], the bin looks to the RIGHT: q = j + 1, and
 *             while q < K - 1 and m[q] < m[q+1], q = q + 1; the owner is q if q is a peak, else there is none.  Otherwise, if
 *             j > 0 and m[j] < m[j-1], it looks to the LEFT the same way: q = j - 1, and while q > 0 and m[q] < m[q-1],
 *             q = q - 1; the owner is q if q is a peak, else none.  Otherwise none.  The side is chosen by the bin's own two
 *             comparisons alone: a trough ascends to both sides and belongs to the right; if its walk to the right ends on a
 *             plateau it has no owner (it does not try the left).  Plateaus, the bins of a ramp that ends at 0 or K - 1,
 *             silent frames and NaN cells have none.
 *     a peak k:             v = acc[k] + inc[k];  new[k] = v - rintf(v)
 *     bin j owned by k != j: w = new[k] + (((j - k) & 1) ? 0.5f : 0.0f);  new[j] = w - rintf(w)      (the bins of a main lobe
 *             alternate by half a turn: the frame's time origin is its first sample and the window is symmetric)
 *     a bin without owner:  new[j] = acc[j]
 *     phase[b][k][t] = 6.2831855f * new[k];  acc = new
 * so |phase| <= pi (1 + 2^-23).  No atomics, no scratch, no communication between workgroups.
 * FT_EINVAL before any device call: magnitude or phase NULL, B, T or hop < 1, hop > n_fft, B > 65535, K * T beyond 2^31 - 257.
 * FT_EUNSUPPORTED: n_fft not a power of two in 256 .. 4096. */
int ft_spsi_phase(const float* magnitude, float* phase, const int32_t* n_frames, int B, int n_fft, int hop, int T, void* stream);

/* ---- scoring utterances: per-frame log-likelihood and attention diagnostics (csrc/score.hip; additive, not in the reference;
 * functions added at ABI 15, no layout changes) ----------
 * frame_loglik: the exact log-density of every mel frame under the flow, in natural time, and per-utterance totals.  z [T][B][M]
 * fp32 contiguous as the forward leaves it; log_s = HOST array of n_ls (1 ..= 8) device pointers to [T][B][M] views with row
 * stride ld_ls (the convention of flowtron_loss_fwd); reversed = HOST array of n_ls ints, != 0 where flow f's log_s is in that
 * flow's reversed time (an AR_Back_Step: the utterance is flipped about its OWN length; z comes back flipped to natural time,
 * log_s does not); out_lens [B] device int32.  With n_b = min(max(out_lens[b], 0), T), for t < n_b
 *     ll[b][t] = -sum_m z[t][b][m]^2 / (2 sigma^2) - (M / 2) ln(2 pi sigma^2) + sum_f sum_m log_s_f[tau_f(t)][b][m]
 *     tau_f(t) = reversed[f] ? n_b - 1 - t : t
 * frame_ll [B][T] float64, 0 at and behind n_b; total [B] float64 = sum_t ll[b][t].  Nothing at or behind out_lens[b] is read.
 * Arithmetic: float64 on the fp32 inputs converted exactly, every operation rounded on its own (nothing is contracted into a
 * fused multiply-add; z^2 is exact in float64 anyway), no transcendental function on the device, in this order:
 *     lane l = 0 .. 63 owns the channels l and l + 64:   q_l = (0 + z[l]^2) + z[l + 64]^2      (a channel >= M is left out)
 *                                                        s_l = 0;  for f ascending: s_l = s_l + log_s_f[l]; s_l = s_l + log_s_f[l + 64]
 *     the lanes meet in the butterfly  v_l = v_l + v_{l xor off}  for off = 32, 16, 8, 4, 2, 1:  Q from q, S from s
 *     ll = ((-(Q * inv)) - c) + S        inv = 1.0 / (2.0 * sigma * sigma),  c = (M * 0.5) * log((6.283185307179586 * sigma) * sigma),
 *                                        both formed on the host in double (libm's log)
 *     total: p_i = ((0 + ll[i]) + ll[i + 256]) + ...  for i = 0 .. 255, then  p_i = p_i + p_{i + h}  for h = 128, 64, .., 1 and i < h;
 *            total = p_0
 * The orders depend on M and n_b alone -- not on B, T, the grid or the utterance's position -- so utterance b gives the same
 * bits alone as inside any batch, and a float64 replay on the host gives the same bits.  Two launches; no atomics, no scratch.
 * FT_EINVAL before any device call: a NULL pointer (an entry of log_s included), n_ls outside 1 ..= 8, M outside 1 ..= 128,
 * ld_ls < M, T or B < 1, B > 65535, sigma not a positive finite number whose inv is finite.
 *
 * attn_diagnostics: the health of attention maps, one launch for all flows and utterances.  attn: fp32 with ELEMENT strides
 * (flow, utterance, frame, token), so any [F][B][T][L] view is read in place, in NATURAL time; in_lens / out_lens [B] device int32,
 * clamped inside the kernel to l = 1 ..= L tokens and n = 1 ..= T frames; nothing at or behind them is read.  Per (f, b):
 *     peak[t] = the lowest index j < l whose value is largest: from value -inf and no index, j ascending, replace only where
 *               row[j] > value -- a NaN never wins; a row with nothing above -inf (all zero rows do have: 0 > -inf picks j = 0;
 *               all -inf or NaN rows) peaks at 0.   pmax[t] = row[peak[t]]
 *     peaks [F][B][T] int32, -1 at and behind n
 *     counters [F][B][6] int32:  [0] n_attended  = distinct tokens that are some frame's peak
 *                                [1] n_backward  = #{t >= 1: peak[t] < peak[t-1]}
 *                                [2] n_skipped   = sum_{t >= 1} max(peak[t] - peak[t-1] - 1, 0)       (held at 2^31 - 1)
 *                                [3] longest_run = the longest stretch of consecutive frames with one peak
 *                                [4] first_peak = peak[0]      [5] last_peak = peak[n-1]
 *     focus_sum [F][B] float64 = sum_t pmax[t]: with 16 waves to the workgroup, wave w adds the frames w, w + 16, .. ascending
 *                                from 0 in float64, then the 16 partial sums are added in wave order from 0
 * The counters follow from peaks in integer arithmetic.  work: one bit per token, attn_diagnostics_workspace_bytes bytes (host
 * arithmetic only; 0 for a size < 1), 4-byte aligned; contents need not be initialised (integer atomic-or inside a workgroup's
 * own words; no float atomics).  Any T and L.
 * FT_EINVAL before any device call: a NULL pointer, F, B, T or L < 1, F > 65535, a negative stride, work misaligned or
 * work_bytes too small. */
int ft_frame_loglik(const float* z, const float* const* log_s, const int32_t* reversed, int n_ls, int64_t ld_ls,
                    const int32_t* out_lens, double sigma, double* frame_ll, double* total, int T, int B, int M, void* stream);
size_t ft_attn_diagnostics_workspace_bytes(int F, int B, int L);
int ft_attn_diagnostics(const float* attn, int64_t stride_f, int64_t stride_b, int64_t stride_t, int64_t stride_l,
                        const int32_t* in_lens, const int32_t* out_lens, int32_t* peaks, int32_t* counters, double* focus_sum,
                        void* work, size_t work_bytes, int F, int B, int T, int L, void* stream);

/* ---- endpoints and loudness of a zero-padded batch (csrc/level.hip; additive, not in the reference, which only divides by the
 * peak at the end of inference.py; functions added at ABI 15, no layout changes) ----------
 * Common to the three entries: audio is fp32 with ELEMENT strides (utterance, sample), read in place; n_samples [B] device int32,
 * clamped inside the kernels to n = 1 ..= N; nothing at or behind n is read; utterance b gives the same bits alone as inside any
 * batch.  start / end [B] device int32 (either may be NULL: 0 and n) name the span s = min(max(start, 0), n - 1),
 * e = min(max(end, s + 1), n) of len = e - s >= 1 samples.  float64 arithmetic is on the fp32 samples converted exactly, every
 * operation rounded on its own (nothing is contracted into a fused multiply-add), no transcendental function on the device.
 *
 * level_bounds (two launches): T = N / hop + 1 frames, utterance b has n / hop + 1.  Frame t holds the F = frame_length samples
 * from t hop - F / 2 on, samples outside [0, n) count as 0 (librosa.effects.trim's centred framing; unpinned against librosa):
 *     lane l = 0 .. 63:   q_l = 0;  for j = l, l + 64, .. < F ascending:  q_l = q_l + x^2      (float64; x^2 is exact)
 *     the lanes meet in the butterfly  q_l = q_l + q_{l xor off}  for off = 32, 16, 8, 4, 2, 1;   power[b][t] = fp32(Q / F)
 *     frame_peak[b][t] = max |x[i]| over t hop <= i < min((t + 1) hop, n)          (both 0 for t > n / hop)
 *     ref = ref_power where it is > 0, else max_t power[b][t];   frame t is active iff  double(power) > double(threshold) * double(ref)
 *     (the product of two fp32 is exact in float64).  With first / last the lowest / highest active frame:
 *     start = max(first hop - pad, 0),  end = min((last + 1) hop + pad, n);   no active frame, or start >= end (the one active
 *     frame is centred on the utterance's end): start = 0, end = n.   peak[b] = max_t frame_peak[b][t] = max |x| over [0, n), exact.
 * power and frame_peak are [B][T] fp32, peak [B] fp32, start / end [B] int32.
 *
 * level_loudness (four launches): ITU-R BS.1770-4 integrated loudness of the span, one channel.  coef (HOST, 7 doubles) = the
 * shelf's b0 b1 b2 a1 a2 and the high pass's a1 a2 (its b is 1, -2, 1) for the sampling rate; per sample x of the span, from a
 * zero state at the span's first sample,
 *     v = (((b0 x + b1 x1) + b2 x2) - a1 v1) - a2 v2              x1, x2 and v1, v2: the previous two inputs and shelf outputs
 *     y = (((v - 2 v1) + v2) - h1 y1) - h2 y2                     y1, y2: the previous two outputs
 * run as a chunked recurrence over chunks of FT_LEVEL_CHUNK = 256 samples, the state s = (v1, v2, y1, y2):
 *     1. every chunk c from s = 0 (x1, x2 are the true samples before the chunk) -> its end state z[c]
 *     2. s[0] = 0;  s[c + 1][r] = z[c][r] + (((M[r][0] s[c][0] + M[r][1] s[c][1]) + M[r][2] s[c][2]) + M[r][3] s[c][3])
 *        carry (HOST, 16 doubles, row-major) = M: column j is the state after 256 steps of the recurrence with x = 0 from the j-th
 *        unit state
 *     3. every chunk again from s[c]; acc = acc + y^2 ascending from 0, restarted at a step boundary: a chunk gives one partial
 *        sum to the step of its first sample and one to the next (step >= 256, so no third)
 *     step_sums[b][k], k < len / step = the partial sums of step k's samples added ascending from 0, in sample order
 *     block j < max(len / step - 3, 0):  z_j = ((S_j + S_{j+1}) + (S_{j+2} + S_{j+3})) / double(4 step)
 *     G1 = {j: z_j > abs_gate};  rel = 0.1 * (sum_{G1} z_j / |G1|);  G2 = {j in G1: z_j > rel};  power = sum_{G2} z_j / |G2|
 *        (both sums ascending from 0);  no block: NaN;  G1 empty: 0
 * step_sums [B][max(N / step, 1)] float64 (0 behind an utterance's steps), power [B] float64, peak [B] fp32 = max |x| over the
 * span.  work: level_loudness_workspace_bytes bytes (host arithmetic only; 0 for a size < 1), 8-byte aligned, need not be
 * initialised.  level_gather (one launch): out [B][N] fp32 contiguous, out[b][i] = fp32(gain[b] * x[s + i]) for i < len (the plain
 * sample where gain is NULL), 0 behind; n_out[b] = len.
 * FT_EINVAL before any device call: a NULL pointer (but start, end, gain), B or N < 1, B > 65535, a negative stride, frame_length
 * odd or < 2, hop outside 1 ..= frame_length, a threshold or ref_power that is negative or not finite, pad < 0, step < 1,
 * abs_gate negative or not finite, a coefficient that is not finite, work misaligned or work_bytes too small.
 * FT_EUNSUPPORTED: frame_length > FT_LEVEL_MAX_FRAME; step < FT_LEVEL_CHUNK (a sampling rate below 2560 Hz) or more than
 * FT_LEVEL_MAX_STEPS steps in N (409.6 s).
 * Measured: the replay of the three passes against scipy.signal.lfilter in float64, 1.9e-14 .. 1.5e-11 relative rms (8, 22.05,
 * 48 kHz; chunks of 64 and 256); a full-scale 997 Hz sine at 48 kHz -3.0103 LUFS; on one MI355X, 64 utterances of 220,672
 * samples: level_bounds 0.08 ms, level_loudness 0.29 ms (filter passes 85 + 90 us, carry 70 us, gate 11 us), the gather 17 us
 * (profiles/level_prof.txt).  Not compared with librosa or any loudness library: neither was available. */
#define FT_LEVEL_CHUNK 256
#define FT_LEVEL_MAX_STEPS 4096
#define FT_LEVEL_MAX_FRAME 4096
int ft_level_bounds(const float* audio, int64_t stride_b, int64_t stride_n, const int32_t* n_samples, float* power,
                    float* frame_peak, float* peak, int32_t* start, int32_t* end, int B, int N, int frame_length, int hop,
                    float threshold, float ref_power, int pad, void* stream);
size_t ft_level_loudness_workspace_bytes(int B, int N);
int ft_level_loudness(const float* audio, int64_t stride_b, int64_t stride_n, const int32_t* n_samples, const int32_t* start,
                      const int32_t* end, const double* coef, const double* carry, double abs_gate, double* step_sums,
                      double* power, float* peak, void* work, size_t work_bytes, int B, int N, int step, void* stream);
int ft_level_gather(const float* audio, int64_t stride_b, int64_t stride_n, const int32_t* n_samples, const int32_t* start,
                    const int32_t* end, const float* gain, float* out, int32_t* n_out, int B, int N, void* stream);

/* ---- pitch and pace of a zero-padded batch: time-domain pitch-synchronous overlap-add on the F0 track (csrc/prosody.hip;
 * additive, the reference has no F0 input; functions added at ABI 15, no layout changes) ----------
 * Two-period Hann grains are cut at analysis marks one period apart and laid down again at a new spacing: the fundamental
 * changes, the spectral envelope stays.  Common to both entries: n_samples [B] device int32, clamped inside the kernels to
 * n = 1 ..= N; nothing at or behind n is read; utterance b gives the same bits alone as inside any batch.  Positions are
 * integers in units of 1 / Q sample, Q = FT_PSOLA_Q = 256; >> is the arithmetic shift, / on integers truncates; fp32 operations
 * are rounded one at a time (nothing is contracted into a fused multiply-add), divisions correctly rounded, rint rounds halves
 * to even.
 *
 * psola_marks (one launch, a wave per utterance).  f0 [B][T] fp32 Hz with ELEMENT strides (utterance, frame), frame t centred
 * on sample t hop, T >= N / hop + 1 (further frames are never read, nor is a frame above n / hop); ratio likewise (a stride may
 * be 0: one factor per utterance, or one for all); pace_q [B] device int32 = the pace in 1 / 65536, clamped to 16384 ..= 262144.
 *   1. a frame is voiced iff 0 < f0[t] < inf (NaN is not).   voiced:   per[t] = int(min(max(rint(sr256 / f0[t]), 16 Q), 1024 Q)),
 *      sr256 = fp32(256 sr);  r = ratio[t], 0.625 where not r >= 0.625, 2 where r > 2;  step[t] = max(8 Q, int(rint(float(per[t]) / r)))
 *      unvoiced: per[t] = step[t] = unvoiced_period Q.        frame(p) = min(T - 1, ((p >> 8) + hop / 2) / hop)
 *   2. analysis marks:  a_0 = 0,  a_{k+1} = a_k + per[frame(a_k)]  while (a_k >> 8) < n;  K of them.  The waveform is not searched
 *      for glottal pulses: neighbouring marks exactly one period apart is what matters, and the sum gives that.
 *   3. n_out = min(N_out, max(1, (n << 16) / pace_q)) in 64 bits.  synthesis marks:  s_0 = 0, k = 0;  while (s_j >> 8) < n_out:
 *        ta = (s_j pace_q) >> 16 (64 bits);  k advances while k + 1 < K and |a_{k+1} - ta| <= |a_k - ta|;
 *        synthesis[j] = s_j,  source[j] = k,  half[j] = (per[frame(a_k)] + 128) >> 8;   s_{j+1} = s_j + step[frame(ta)];  J of them.
 * analysis [B][KA], KA >= ceil(N / 16); synthesis, source, half [B][KS], KS >= ceil(N_out / 8); n_analysis (K), n_synthesis (J),
 * n_out [B]: device int32; entries behind K and J are not written.
 *
 * psola_synth (one launch, a workgroup per 256 output samples).  audio fp32 with ELEMENT strides (utterance, sample), read in
 * place; hann [FT_PSOLA_HANN + 1] device fp32, H[i] = fp32(0.5 + 0.5 cos(pi i / 1024)) formed in float64 on the host.
 *   4. c_j = (s_j + 128) >> 8,  m_j = (a_{source[j]} + 128) >> 8.  Output sample o < n_out takes the grains with |o - c_j| < half[j]
 *      in ascending j, from y = wsum = 0:   d = o - c_j;  w = H[(|d| 1024) / half[j]];  wsum = wsum + w;  y = y + w x[m_j + d]
 *      (x outside [0, n) counts as 0 and is not read);   out[o] = y / wsum where wsum >= 2^-10, else 0.
 * out [B][N_out] fp32 contiguous, 0 at and behind n_out.  With ratio = 1 and pace_q = 65536 the synthesis marks are the analysis
 * marks, source[j] = j, every grain reads the sample it writes, and |out - x| <= 1e-6 for |x| <= 1 (two or three products, their
 * sum and one division: about three units in the last place).
 * FT_EINVAL before any device call: a NULL pointer, B, N, N_out, T or hop < 1, B > 65535, a negative stride, T < N / hop + 1,
 * KA or KS too small, sr256 not positive and finite.  FT_EUNSUPPORTED: N or N_out > FT_PSOLA_MAX_SAMPLES (positions stay below
 * 2^31), unvoiced_period outside FT_PSOLA_MIN_PERIOD ..= FT_PSOLA_MAX_PERIOD.
 * Measured: profiles/prosody_prof.txt.  Not compared with any outside PSOLA implementation: none was available.  The tests pin
 * F0, envelope, length and bits, not how it sounds. */
#define FT_PSOLA_Q 256
#define FT_PSOLA_MIN_PERIOD 16
#define FT_PSOLA_MAX_PERIOD 1024
#define FT_PSOLA_MAX_SAMPLES (1 << 22)
#define FT_PSOLA_HANN 1024
int ft_psola_marks(const float* f0, int64_t f0_stride_b, int64_t f0_stride_t, const float* ratio, int64_t ratio_stride_b,
                   int64_t ratio_stride_t, const int32_t* n_samples, const int32_t* pace_q, int32_t* analysis, int32_t* n_analysis,
                   int32_t* synthesis, int32_t* source, int32_t* half, int32_t* n_synthesis, int32_t* n_out, int B, int N,
                   int N_out, int T, int hop, int KA, int KS, float sr256, int unvoiced_period, void* stream);
int ft_psola_synth(const float* audio, int64_t stride_b, int64_t stride_n, const int32_t* n_samples, const int32_t* analysis,
                   const int32_t* synthesis, const int32_t* source, const int32_t* half, const int32_t* n_synthesis,
                   const int32_t* n_out, const float* hann, float* out, int B, int N, int N_out, int KA, int KS, void* stream);

/* ---- a pace that varies within the utterance: the synthesis marks walk a time map (csrc/prosody.hip; additive; functions
 * added at ABI 15, no layout changes).  psola_synth lays the grains down from these marks unchanged ----------
 * psola_marks_warp (one launch, a wave per utterance) is psola_marks with three differences; steps 1 and 2, per[], frame(p),
 * the analysis marks, the source choice, half, the units and the fp32 discipline are word for word the block's above.
 *   a. n_out_in [B] device int32 is given: n_out = min(max(n_out_in, 1), N_out).  There is no pace_q.
 *   b. tmap [B][TM] device int32, contiguous, TM >= N_out / hop_out + 2: tmap[u] is the input position, in 1 / Q sample, that
 *      output sample u hop_out plays.  For mark s_j, in 64 bits:   u = (s_j >> 8) / hop_out,  fr = s_j - u hop_out Q,
 *        lin = tmap[u] + ((tmap[u + 1] - tmap[u]) fr) / (hop_out Q)          (/ truncates toward zero)
 *        ta_j = min(max(lin, ta_{j-1}, 0), Q n - 1),  ta_{-1} = 0
 *      The running maximum makes any map monotone as the walk sees it (a decreasing stretch holds the input still); the
 *      clamp keeps every read in range whatever the map holds.  ta_j takes the place of (s_j pace_q) >> 16 in step 3.
 *   c. ratio [B][RT] fp32 with element strides.  ratio_axis = 0: r_j = ratio[frame(ta_j)], the input's frame, RT >= N / hop + 1.
 *      ratio_axis = 1: r_j = ratio[min(RT - 1, ((s_j >> 8) + hop_out / 2) / hop_out)], the OUTPUT's frame (a target contour lives
 *      there), RT >= N_out / hop_out + 1.  r_j is clamped as in step 1 (0.625 where not r >= 0.625, 2 where r > 2).  As no frame
 *      of f0 above n / hop is read, no entry of ratio above n_out / hop_out is (the index stops there), nor one of tmap above
 *      (n_out - 1) / hop_out + 1: an utterance gives the same bits alone as in a longer batch.
 *      frame(ta_j) voiced:  s_{j+1} = s_j + max(8 Q, int(rint(float(per[frame(ta_j)]) / r_j)));  unvoiced:  s_j + unvoiced_period Q.
 * The walk ends for any contents of f0, ratio, tmap and n_out_in: every step adds at least 8 Q to s_j, J < KS, K < KA,
 * u <= TM - 2, and ta_j < Q n bounds every frame index.  With tmap[u] = u hop Q pace (hop_out = hop, pace 1, 2 or 0.5),
 * n_out_in = max(1, (n << 16) / pace_q) and ratio_axis = 0 the marks are psola_marks's at that pace, bit for bit.
 * Outputs, KA and KS as psola_marks.  FT_EINVAL before any device call: psola_marks's, and hop_out < 1 or > FT_PSOLA_MAX_SAMPLES,
 * TM < N_out / hop_out + 2, RT too small for the axis, ratio_axis not 0 or 1.  FT_EUNSUPPORTED: psola_marks's.
 *
 * psola_time_map (one launch, a workgroup per utterance): a warping path to such a map.  path [B][P][2] device int32, the cells
 * (i_c, j_c) = (source frame, reference frame) in ascending order as ft_dtw writes them; path_len [B]; P_b = min(max(path_len[b],
 * 1), P); cells at and behind P_b are not read.  i_c is clamped to 0 ..= (FT_PSOLA_MAX_SAMPLES - 1) / hop, j_c to 0 ..= P - 1.
 *   J_b = j_{P_b - 1} + 1;  lo_j / hi_j = the i of the first / last cell of reference frame j (cell c is the first of its j iff
 *   c = 0 or j_{c-1} != j_c, the last iff c = P_b - 1 or j_{c+1} != j_c: one plain store each, no atomics; a j no cell names
 *   has lo_j = hi_j = 0, which no path of ft_dtw leaves);   mid_j = 128 hop (lo_j + hi_j)   (the middle of the matched source
 *   frames, in 1 / Q sample);   tmap[u] = (sum over d = -w ..= w of mid[min(max(u + d, 0), J_b - 1)]) / (2 w + 1) for 0 <= u < TM,
 *   in 64 bits, truncating.  tmap [B][TM] is nondecreasing wherever j_c does not descend and i_c does not either.
 * FT_EINVAL: a NULL pointer, B, P, TM or hop < 1, B > 65535, hop > FT_PSOLA_MAX_SAMPLES, w outside 0 ..= FT_PSOLA_MAX_SMOOTH.
 * FT_EUNSUPPORTED: P > FT_PSOLA_MAX_PATH (mid[] lives in LDS).
 * Measured: profiles/prosody_warp_prof.txt.  tests/prosody_warp_ref.py replays both bit for bit. */
#define FT_PSOLA_MAX_PATH 4096
#define FT_PSOLA_MAX_SMOOTH 32
int ft_psola_marks_warp(const float* f0, int64_t f0_stride_b, int64_t f0_stride_t, const float* ratio, int64_t ratio_stride_b,
                        int64_t ratio_stride_t, const int32_t* n_samples, const int32_t* n_out_in, const int32_t* tmap,
                        int32_t* analysis, int32_t* n_analysis, int32_t* synthesis, int32_t* source, int32_t* half,
                        int32_t* n_synthesis, int32_t* n_out, int B, int N, int N_out, int T, int RT, int TM, int hop, int hop_out,
                        int ratio_axis, int KA, int KS, float sr256, int unvoiced_period, void* stream);
int ft_psola_time_map(const int32_t* path, const int32_t* path_len, int32_t* tmap, int B, int P, int TM, int hop, int w,
                      void* stream);

/* ---- F0-adaptive spectral envelope and its mel-cepstrum (CheapTrick: Morise, "CheapTrick, a spectral envelope estimator for
 * high-quality speech synthesis", Speech Communication 2015; the frequency transform of SPTK; csrc/envelope.hip; additive, the
 * reference has no metric; a function added at ABI 15, no layout changes) ----------
 * One launch, a workgroup per frame.  audio fp32 with ELEMENT strides (utterance, sample), read in place; n_samples [B] device
 * int32, clamped inside the kernel to n = 1 ..= N; nothing at or behind n is read; utterance b gives the same bits alone as
 * inside any batch.  f0 [B][T_f0] fp32 Hz with ELEMENT strides (utterance, frame), frame t centred on sample c = t hop,
 * T_f0 >= T = N / hop + 1 (further frames are never read, nor is a frame above n / hop).  fft_size = 512, 1024 or 2048,
 * H = fft_size / 2, df = sr / fft_size (exact: sr is an integer rate held in fp32).  sr15 = fp32(1.5 sr).
 * This is CheapTrick as published with the two random-noise safeguards of the WORLD implementation replaced by one
 * deterministic floor, and with step 5 summed directly (below).
 *
 * The integers.  Every integer the rule takes from F0 is formed from the fp32 f0 by these fp32 operations, each correctly rounded
 * (no fast division, nothing contracted), so a float64 replay that forms them with fp32 takes the same window and the same bins:
 *   f    = f0[t]  if  f0_floor <= f0[t] <= 1000  (NaN, infinities, 0 and negatives fail it),  else 500
 *   half = min(int(floor(sr15 / f + 0.5)), H - 1)                 (the min never binds where fft_size follows from f0_floor)
 *   wq   = f / df;          ul = min(2 + int(wq), H)
 *   wb   = ((2 f) / 3) / df;     bnd = int(wb) + 1;     hw = 0.5 wb + 0.5;     n_w = min(int(hw), H);     fr = hw - float(n_w)
 *   wd   = 2 hw - 1        (exact, as fr is: the smoothing width in bins, 2 f / (3 df) as hw holds it, within an fp32 ulp of wb)
 * f, wq, wd and fr enter the real-valued steps as these fp32 values.  What follows is real arithmetic: the kernel's is fp32 (three
 * sums of step 2 and the phases of steps 2 and 6 in float64), the replay's float64; neither order nor rounding is pinned.
 *   2. window.  i = -half ..= half:  idx = min(max(c + i, 0), n - 1)  (edge replication against the utterance's OWN n);
 *      w_i = 0.5 cos(pi i f / sr15) + 0.5;   s_i = (x[idx] w_i - w_i (sum_i x[idx] w_i / sum_i w_i)) / sqrt(sum_i w_i^2)
 *   3. P[k] = |DFT_{fft_size}(s zero-padded)[k]|^2,  k = 0 ..= H.
 *   4. DC correction.  For k < ul - 1:  pos = wq - k (exact in fp32), j = int(pos), g = pos - j;
 *      P'[k] = P[k] + P[j] + g (P[j + 1] - P[j])  -- the interpolation reads the uncorrected P.  P'[k] = P[k] elsewhere.
 *   5. smoothing over width = wd df.  With the mirror  M[j] = P'[-j] for j < 0,  P'[2 H - j] for j > H,  P'[j] otherwise
 *      (WORLD mirrors bnd bins at both ends; n_w <= bnd), S[k] is the mean over [k - wd / 2, k + wd / 2] (in bins) of the
 *      piecewise-constant function that holds M[j] on [j - 1/2, j + 1/2), summed DIRECTLY:
 *        S[k] = (sum_{j = k - n_w + 1}^{k + n_w - 1} M[j]  (ascending)  + fr (M[k - n_w] + M[k + n_w])) / wd + 1e-20
 *      (n_w = 0: S[k] = P'[k] + 1e-20).  The difference of two values of a cumulative sum, WORLD's form, is the same number in
 *      exact arithmetic and cancels in fp32: a prefix sum the size of the frame's power has an ulp at -72 dB of it.
 *   6. liftering.  c2[q] = (1 / fft_size) sum_k L[k] cos(2 pi k q / fft_size) over the even extension L of log S, q = 0 ..= H;
 *      for q >= 1, x = f q / sr:  c2[q] *= sin(pi x) / (pi x) ((1 - 2 q1) + 2 q1 cos(2 pi x)).
 *      env[k] = exp(sum_q c2[q] cos(2 pi k q / fft_size) over the even extension of c2),  the POWER envelope.
 *   7. mel-cepstrum.  c^[0] = c2[0] / 2, c^[q] = c2[q], c^[H] = c2[H] / 2 (the one-sided cepstrum of the log AMPLITUDE);
 *      mc[m] = sum_q A[m][q] c^[q], m = 0 ..= order: lane l = 0 .. 63 adds q = l, l + 64, .. ascending and the lanes meet in the
 *      butterfly acc_l + acc_{l xor off}, off = 32 .. 1.  A = freqt [order + 1][H + 1] device fp32: the matrix of SPTK's frequency
 *      transform for alpha, made on the host in float64 by running its recursion over i = H .. 0 on unit vectors
 *      (g_0 = c_i + a d_0;  g_1 = (1 - a^2) d_0 + a d_1;  g_j = d_{j-1} + a (d_j - g_{j-1})) and rounded once.
 * twiddle [3 fft_size / 4][2] device fp32: (cos, -sin)(2 pi j / fft_size), float64 rounded once.
 * env [B][T][H + 1] and mc [B][T][order + 1] fp32 contiguous; either may be NULL (not computed, not written: without env the third
 * transform is not run); rows t > n / hop are 0.
 * FT_EINVAL before any device call: a NULL pointer (but one of env, mc; freqt without mc), B, N or hop < 1, B > 65535, a negative
 * stride, T_f0 < N / hop + 1, sr, sr15 or q1 not finite or sr not positive, f0_floor outside 0 < f0_floor <= 1000, order outside
 * 1 ..= FT_ENVELOPE_MAX_ORDER or >= H, a window at f0_floor longer than fft_size, 1000 / df + 2 > min(H, 250).
 * FT_EUNSUPPORTED: another fft_size.
 * Measured: profiles/envelope_prof.txt.  NOT pinned against pyworld or pysptk: neither was available. */
#define FT_ENVELOPE_MAX_ORDER 32
int ft_spectral_envelope(const float* audio, int64_t stride_b, int64_t stride_n, const int32_t* n_samples, const float* f0,
                         int64_t f0_stride_b, int64_t f0_stride_t, const float* twiddle, const float* freqt, float* env, float* mc,
                         int B, int N, int T_f0, int hop, int fft_size, int order, float sr, float sr15, float f0_floor, float q1,
                         void* stream);

/* ---- attention-CTC loss (flowtron.py:155-182, 245-274) ------------------------------
 * lp [B,T,L] = attn_logprob in natural time order.  Per sample: classes {blank (logit blank_logprob), 1..K_b} with
 * K_b = in_lens[b], frames t < out_lens[b]; log_softmax over the classes, CTC against the target 1..K_b (blank 0),
 * reduction 'mean' (divide by K_b), zero_infinity, then the batch mean.  loss[0] receives the scalar.  work holds
 * alpha and beta [B,T,2L+1], the log-softmax normalisers [B,T] and nll [B] (ft_attn_ctc_workspace_floats floats).
 * with_beta != 0: the beta recursion runs beside alpha in the same launch (a second workgroup per sample; both are
 * latency-bound in T), so the backward pass is a single elementwise kernel -- pass beta_ready = with_beta to bwd.
 * bwd: dlp [B,T,L] = gout_dev[0] * d loss / d lp (overwritten; zero outside the valid [T_b, K_b] window). */
size_t ft_attn_ctc_workspace_floats(int B, int T, int L);
int ft_attn_ctc_fwd(const float* lp, const int32_t* in_lens, const int32_t* out_lens, float blank_logprob,
                    float* work, float* loss, int B, int T, int L, int with_beta, void* stream);
int ft_attn_ctc_bwd(const float* lp, const int32_t* in_lens, const int32_t* out_lens, float blank_logprob,
                    float* work, const float* gout_dev, float* dlp, int B, int T, int L, int beta_ready, void* stream);
/* The same loss over F flows at once (FlowtronLoss, flowtron.py:245-274: the per-flow losses averaged): F * B stacked samples,
 * sample f * B + b = flow f's log-probabilities of utterance b; loss[0] = mean over flows of the per-flow batch means.  lp / dlp:
 * HOST arrays of F (<= 8) device pointers to [B,T,L] tensors; reversed[f] != 0 (host array): flow f's tensor is in REVERSED time
 * (an AR_Back_Step: frame t of utterance b is row out_lens[b] - 1 - t) -- the reference flips + rolls the tensor there and back
 * (:250-271), here the row index is mirrored in the kernels, for the loss and for dlp[f] (which comes out in the flow's own order).
 * No concatenated or re-reversed copy exists.  work: ft_attn_ctc_workspace_floats(F * B, T, L) floats.  (ABI 12) */
int ft_attn_ctc_fwd_multi(const float* const* lp, const int32_t* reversed, int F, const int32_t* in_lens, const int32_t* out_lens,
                          float blank_logprob, float* work, float* loss, int B, int T, int L, int with_beta, void* stream);
int ft_attn_ctc_bwd_multi(const float* const* lp, const int32_t* reversed, int F, const int32_t* in_lens, const int32_t* out_lens,
                          float blank_logprob, float* work, const float* gout_dev, float* const* dlp, int B, int T, int L,
                          int beta_ready, void* stream);

/* ---- cumulative ("location-sensitive") attention of a teacher-forced flow, one call per sequence ----------
 * flowtron.py:697-723 (run_cumm_attn_sequence), :129-152 (AttentionConditioningLayer), :544-592 (Attention.forward).  Per frame
 * i: cond = sigmoid(conv_K2(relu(conv_K1([cumm_i ; prev_i])))) over the text axis (2 -> NF -> E channels, zero padding at the ends),
 * keys = (text . cond) w_key^T, scores v . tanh(Q_i + keys) / temperature, softmax over l < in_lens[b], logprob = log(attn + 1e-8),
 * ctx_i = attn_i V, cumm_{i+1} = cumm_i + attn_i, prev_{i+1} = attn_i.  The LIBRARY walks the T dependent frames, enqueued back to
 * back on `stream`, no host synchronisation:
 *   - 16-bit operand modes at the config.json width (E = A = 640, NF 32, K1 5, K2 3; ft_cumm_attn_fused() != 0, ABI 11): ONE fused
 *     launch per frame and direction (csrc/cumm_fused.hip); context, dV, dctx . V and every weight gradient leave the frame loop
 *     and run as a few large GEMMs over all frames (the backward keeps 16-bit streams of dK / km / dpre2 / col2 for a chunk of
 *     frames in `work`).  kproj_all then holds tanh(Q_i + K_i) of the rows l < in_lens[b] instead of K_i.
 *   - otherwise (fp32 parity mode, other widths, FT_CUMM_FUSED=0): a chain of 8 launches per frame forward, 22 backward.
 * Layouts: text [L][B][E] (encoder outputs), Q [T][B][A] and V [L][B][A] (already projected), w_key [A][E], v [A], w1 [NF][2][K1],
 * w2 [E][NF][K2]; outputs ctx [T][B][A], attn / logprob [B][T][L].  Saved for backward (caller-owned, filled by fwd):
 * cumm_all [T][B][L] and kproj_all [T][L*B][A].  work: ft_cumm_attn_workspace_bytes() bytes, 256-byte aligned.
 * bwd: dctx [T][B][A]; dattn / dlogprob [B][T][L] or NULL; every gradient output is overwritten (accumulated over the frames
 * inside): dQ [T][B][A], dV [L][B][A], dtext [L][B][E], dw_key, dv, dw1, db1, dw2, db2. */
typedef struct {
    const float *text, *Q, *V, *w_key, *v, *w1, *b1, *w2, *b2;
    const int32_t* in_lens;
    float *ctx, *attn, *logprob, *cumm_all, *kproj_all;
    void* work; size_t work_bytes;
    int T, B, L, E, A, NF, K1, K2;
    float temperature;
    int mode;
    /* optional (ABI 11): a device status word (zeroed by the caller once; the one the persistent recurrences use will do).  When given,
     * and the fused path's work list is co-resident by construction (B x ceil(L / 32) <= CUs), the forward frames run as ONE
     * persistent launch (per-utterance granule hand-offs instead of a launch boundary per frame); *persist_status becomes non-zero if
     * a hand-off wait gives up (grid not co-resident: a foreign kernel holds CUs) -- the caller must then not trust the outputs. */
    int32_t* persist_status;
} ft_cumm_attn_args;
size_t ft_cumm_attn_workspace_bytes(int T, int L, int B, int E, int A, int NF, int K1, int K2, int mode, int backward);
int ft_cumm_attn_fused(const ft_cumm_attn_args* a);     /* 1: fwd / bwd of these arguments take the fused one-launch-per-frame path */
/* debug: device buffer [2][4096][16] int64 that later fused launches fill with stage stamps of workgroup (0, 0) (100 MHz clock;
 * [0] = forward, [1] = backward, second index = frame); NULL switches it off (scripts/exp/cumm_prof.py) */
int ft_cumm_attn_debug_prof(void* dev_buf);
int ft_cumm_attn_fwd(const ft_cumm_attn_args* a, void* stream);
int ft_cumm_attn_bwd(const ft_cumm_attn_args* a, const float* dctx, const float* dattn, const float* dlogprob,
                     float* dQ, float* dV, float* dtext, float* dw_key, float* dv, float* dw1, float* db1, float* dw2, float* db2,
                     void* stream);

/* ---- beta-binomial attention prior (data.py:31-41, 111-141) --------
 * prior[b,t,k] = BetaBinom.pmf(k; n = in_lens[b]-1, a = scaling*(t+1), b = scaling*(out_lens[b]-t)) for
 * t < out_lens[b], k < in_lens[b]; 0 in the padding.  [B,T,L] fp32, float64 lgamma inside. */
int ft_beta_binomial_prior(const int32_t* in_lens, const int32_t* out_lens, float* prior,
                           int B, int T, int L, float scaling, void* stream);

/* ---- fused RAdam over a flat arena (radam.py:44-122) + grad-norm clip ----------
 * One pass: g *= min(1, clip / (sqrt(*gnorm_sq_dev) + 1e-6)) (torch clip_grad_norm_, train.py:328; skipped when clip == 0
 * or gnorm_sq_dev == NULL), v = beta2 v + (1-beta2) g g, m = beta1 m + (1-beta1) g, p -= weight_decay*lr*p,
 * p -= step_size * (rectified ? m / (sqrt(v) + eps) : m).  step_size is radam.py:95-105 (contains lr).  Hyper-parameters
 * are doubles like the python optimizer's; derived coefficients are rounded to fp32 once.
 * Guard (device side, no host synchronisation): when gnorm_sq_dev is given and *gnorm_sq_dev is NaN or Inf the whole update
 * is SKIPPED -- p, m, v keep their values -- and *skipped_dev (optional) is incremented: what GradScaler.step does for an fp16
 * overflow (train.py:330), extended to every non-finite global norm, so that one poisoned step (ft_poison_if_nonzero below)
 * can never reach the weights or the moments.
 * ft_sumsq: acc[0] += sum x^2, DETERMINISTIC (no float atomics: per-workgroup partial sums into `partials`, FT_SUMSQ_PARTIALS
 * floats of caller scratch, added in index order by one workgroup) -- data-parallel replicas stay bit-identical only if every
 * rank derives the same clip factor from the same reduced gradients. */
#define FT_SUMSQ_PARTIALS 1024
int ft_sumsq(const float* x, float* acc, int64_t n, float* partials, void* stream);
int ft_radam_step(float* p, const float* g, float* m, float* v, int64_t n,
                  const float* gnorm_sq_dev, double clip, double lr, double beta1, double beta2, double eps,
                  double weight_decay, double step_size, int rectified, int32_t* skipped_dev, void* stream);
/* The same update with the step count formed on the device (ABI 12): step = calls - *skipped_dev, where calls = the number of
 * optimizer steps issued so far (this one included) and *skipped_dev the updates the guard has dropped so far; step_size and the
 * rectification switch (radam.py:82-106) are evaluated from it in double inside the kernel.  The schedule then follows the APPLIED
 * updates exactly -- radam.py's state['step'] under GradScaler, which does not call step() after an overflow (train.py:330) --
 * without the host reading the drop decision: an optimizer that sets `_step_supports_amp_scaling` lets torch's GradScaler.step
 * hand over `found_inf` as a device tensor instead of synchronising on it (one host sync per fp16 step gone). */
int ft_radam_step_dev(float* p, const float* g, float* m, float* v, int64_t n, const float* gnorm_sq_dev, double clip,
                      double lr, double beta1, double beta2, double eps, double weight_decay, int calls,
                      int32_t* skipped_dev, void* stream);
/* if (*status_dev != 0) dst[0] = NaN.  Enqueued behind the last persistent recurrence launch of a backward pass on the first
 * element of a gradient bucket BEFORE its all-reduce / the norm reduction: a recurrence that reported a time-out (status word of
 * ft_lstm_persist_*) poisons the global gradient norm on EVERY rank, and the guard of ft_radam_step drops that step everywhere. */
int ft_poison_if_nonzero(const int32_t* status_dev, float* dst, void* stream);

/* ---- Gaussian-mixture prior (flowtron.py:217-231, 312-363, 437-439; csrc/mixture.hip; functions added at ABI 15) --------
 * All fp32, no float atomics: every reduction is two-stage and ordered, so two calls on the same inputs give identical bits.
 * Mixture negative log-likelihood of z [T,B,M] under C components: mean, log_var [Bm,M,C] with Bm = 1 (fixed Gaussians, shared
 * by the batch) or Bm = B, prob [B,C]; with valid = t < out_lens[b] (lengths clamped to 0 ..= T; padded frames are never read),
 *   l[t,b,m] = log sum_c prob[b,c] exp(-(z - mean_c)^2 / (2 exp(log_var_c))) / sqrt(exp(log_var_c))      (no sigma, no 2 pi term)
 *            = lse_c(log prob_c - log_var_c / 2 - (z - mean_c)^2 exp(-log_var_c) / 2), formed in the log domain,
 *   *loss_out = -(sum_valid l + sum_f sum_valid log_s[f]) / (n_valid_frames M).
 * log_s, n_ls (<= 8), ld_ls: as the fused Flowtron loss forward takes them.  acc: 8 floats the backward reads ([4] = 1 / (n M)).
 * work: the float count the work query returns (scratch; forward and backward may share it).  Limits, checked on the host before
 * any device call (FT_EINVAL): 2 <= C <= FT_MIXTURE_MAX_C, Bm in {1, B}, M <= 256, (3 M C + 2 C) floats within 62 KB of LDS.
 * Backward (g: the incoming gradient, one device float): dz [T,B,M] and dls [T,B,M] (the gradient of EVERY log_s; may be NULL),
 * zeros at padded frames; dmean, dlog_var [B,M,C] (per utterance also when Bm = 1: the caller adds the rows), dprob [B,C] -- any
 * of the three may be NULL; work is needed when one is given. */
#define FT_MIXTURE_MAX_C 64
size_t ft_mixture_nll_work_floats(int T, int B, int M, int C);
int ft_mixture_nll_fwd(const float* z, const float* mean, const float* log_var, const float* prob, const float* const* log_s,
                       int n_ls, int64_t ld_ls, const int32_t* out_lens, float* acc, float* work, float* loss_out,
                       int T, int B, int M, int C, int Bm, void* stream);
int ft_mixture_nll_bwd(const float* z, const float* mean, const float* log_var, const float* prob, const int32_t* out_lens,
                       const float* acc, const float* g, float* dz, float* dls, float* dmean, float* dlog_var, float* dprob,
                       float* work, int T, int B, int M, int C, int Bm, void* stream);
/* y[b,c] = sum_{t < lens[b]} x[t,b,c] / max_b lens[b] (x [T,B,W] contiguous; the reference's torch.mean over the time axis of a
 * zero-padded BiLSTM output, flowtron.py:437-439: the divisor is the batch's LONGEST length, found on the device), and its adjoint
 * dx[t,b,c] = dy[b,c] / max_b lens[b] at t < lens[b], 0 beyond. */
int ft_time_pool_fwd(const float* x, const int32_t* lens, float* y, int T, int B, int W, void* stream);
int ft_time_pool_bwd(const float* dy, const int32_t* lens, float* dx, int T, int B, int W, void* stream);
/* softmax over the C (2 ..= FT_MIXTURE_MAX_C) entries of each of B rows, and dx = y (dy - sum_c y_c dy_c) */
int ft_softmax_rows_fwd(const float* x, float* y, int B, int C, void* stream);
int ft_softmax_rows_bwd(const float* y, const float* dy, float* dx, int B, int C, void* stream);
/* out[s,m,t] = mean[row_s,m,k_s] + sigma exp(log_var[row_s,m,k_s] / 2) eps[s,m,t]: S samples [S,M,n_frames] of ONE component each
 * (component: device int32 [S]; rows: device int32 [S] into the Bm rows of mean / log_var, NULL = row 0 with Bm = 1).  eps: the
 * caller's N(0,1) draws (NULL with sigma = 0: the component means).  A row or component outside its range gives NaN, reads nothing. */
int ft_mixture_sample(const float* mean, const float* log_var, const int32_t* rows, const int32_t* component, const float* eps,
                      float* out, int S, int M, int n_frames, int C, int Bm, float sigma, void* stream);

/* ---- fp16-operand twins (FT_F16): same signatures, semantics and workspace queries as the entries they are named after;
 * 16-bit images / fragments made by a twin must only be fed to twins. ---- */
int ft_gemm_f16(const ft_gemm_args* a, void* stream);
int ft_bf16_image_f16(const float* src, int64_t ld, int64_t rows, int64_t cols, void* dst, void* stream);
int ft_bf16_image_colsum_f16(const float* src, int64_t ld, int64_t rows, int64_t cols, void* dst, float* colsum, void* stream);
int ft_gemm_img_f16(const ft_gemm_img_args* a, void* stream);
int ft_gemm_img_group_f16(const ft_gemm_img_args* probs, int n, void* stream);
int ft_bf16_image_rows_f16(const float* src, int64_t ld, int64_t cap_rows, int64_t cols, void* dst, float* colsum,
                           const int32_t* rowmap, const int32_t* rows_dev, void* stream);
int ft_lstm_seq_fwd_f16(const float* gx, const float* w_hh, const int32_t* lens,
                    float* y, int64_t ldy, float* gates, float* cell, void* work,
                    int T, int B, int H, int reverse, int mode, void* stream);
int ft_lstm_seq_bwd_f16(const float* dy, int64_t ldy, const float* w_hh, const int32_t* lens,
                    const float* gates, const float* cell, float* dgx, void* work,
                    int T, int B, int H, int reverse, int mode, void* stream);
int ft_lstm_persist_bwd_f16(const float* dy, int64_t ldy, const float* w_hh, const int32_t* lens, const float* gates,
                        const float* cell, float* dgx, void* work, int32_t* status, int T, int B, int H, int ng, void* stream);
int ft_lstm_persist_bwd_img_f16(const float* dy, int64_t ldy, const float* w_hh, const int32_t* lens, const float* gates,
                            const float* cell, float* dgx, void* work, int32_t* status, int T, int B, int H, int ng,
                            void* dimg, int64_t dimg_ld, int64_t dimg_rows, float* dbias, void* stream);
int ft_lstm_roles_prepare_fwd_f16(const float* w_hh, void* wimg, int H, void* stream);
int ft_lstm_roles_prepare_bwd_f16(const float* w_hh, void* wimg, int H, void* stream);
int ft_lstm_roles_prepare_table_f16(const ft_wfrag_desc* descs, int n, int H, void* stream);
int ft_lstm_roles_fwd_f16(const ft_lstm_fwd_role* roles, int n_roles, int rows_per_group, int reset_rows, void* ctx, int phase,
                          int32_t* status, int H, void* stream);
int ft_lstm_roles_bwd_f16(const ft_lstm_bwd_role* roles, int n_roles, int rows_per_group, int reset_rows, void* ctx, int phase,
                          int32_t* status, int H, void* stream);
int ft_lstm2_seq_fwd_f16(const float* gx0, const float* w_hh0, const float* w_ih1, const float* bias1, const float* w_hh1,
                     const int32_t* lens, float* y0, float* gates0, float* cell0, float* y1, float* gates1, float* cell1,
                     void* work, int T, int B, int H, void* stream);
int ft_lstm2_seq_bwd_f16(const float* dy1, const float* w_hh0, const float* w_ih1, const float* w_hh1, const int32_t* lens,
                     const float* gates0, const float* cell0, const float* gates1, const float* cell1,
                     float* dgx0, float* dgx1, void* work, int T, int B, int H, void* stream);
int ft_lstm_bidir_seq_fwd_f16(const float* gx_f, const float* gx_r, const float* w_hh_f, const float* w_hh_r,
                          const int32_t* lens, float* y, int64_t ldy, float* gates_f, float* gates_r,
                          float* cell_f, float* cell_r, void* work_f, void* work_r, int T, int B, int H, void* stream);
int ft_lstm_bidir_seq_bwd_f16(const float* dy, int64_t ldy, const float* w_hh_f, const float* w_hh_r, const int32_t* lens,
                          const float* gates_f, const float* gates_r, const float* cell_f, const float* cell_r,
                          float* dgx_f, float* dgx_r, void* work_f, void* work_r, int T, int B, int H, void* stream);
int ft_bilstm_persist_fwd_f16(const float* gx_f, const float* gx_r, const float* w_hh_f, const float* w_hh_r, const int32_t* lens,
                          float* y, int64_t ldy, float* gates_f, float* gates_r, float* cell_f, float* cell_r,
                          void* work, int32_t* status, int T, int B, int H, void* stream);
int ft_bilstm_persist_bwd_f16(const float* dy, int64_t ldy, const float* w_hh_f, const float* w_hh_r, const int32_t* lens,
                          const float* gates_f, const float* gates_r, const float* cell_f, const float* cell_r,
                          float* dgx_f, float* dgx_r, void* work, int32_t* status, int T, int B, int H, void* stream);

#ifdef __cplusplus
}
#endif
#endif
