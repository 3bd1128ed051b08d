/*
 * planer_hip.h -- C ABI of libplaner_hip.so, the MI355X (gfx950) backend for
 * planer's per-layer forward pass.
 *
 * The reference (Image-Py/planer v0.34) is pure Python; its "backend" is any
 * module that quacks like numpy, swapped in by planer.core() (__init__.py:22-38).
 * Its only native/GPU call site is cupy.cudnn.convolution_forward
 * (util.py:66-77).  This header is what a ctypes binding for a HIP backend
 * binds instead; every entry point cites the reference function it replaces.
 * INTEGRATION.md shows the reference-side stub.
 *
 * Conventions
 *  - every function returns an int status (PL_OK == 0) and never throws;
 *    pl_last_error() returns a thread-local message for the last failure.
 *  - all tensors are dense fp32, logical layout NCHW, weights OIHW, exactly as
 *    the reference's numpy arrays (layer.py / util.py).
 *  - all pointers named x/y/w/... are DEVICE pointers obtained from pl_alloc;
 *    sizes are element counts unless a name says bytes.
 *  - all work is enqueued on the context's HIP stream and is asynchronous with
 *    respect to the host; pl_sync() waits for it.
 */
#ifndef PLANER_HIP_H
#define PLANER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PL_OK 0
#define PL_EINVAL 1       /* bad argument (null pointer, negative size ...)      */
#define PL_EUNSUPPORTED 2 /* valid in ONNX terms but undefined in the reference, */
                          /* e.g. asymmetric pads (util.py:8), group !| C        */
#define PL_ENOMEM 3
#define PL_EHIP 4         /* a HIP runtime call failed; see pl_last_error()      */
#define PL_ERCCL 5        /* an RCCL call failed                                 */

/* activation codes for the fused conv epilogue */
#define PL_ACT_NONE 0
#define PL_ACT_RELU 1
#define PL_ACT_LEAKY 2
/* OR-ed into an activation code: the fused residual is added AFTER the activation
 * (conv -> batchnorm -> leakyrelu -> add, the order YOLO-v3's blocks use) instead of before it */
#define PL_ACT_RES_AFTER 16

typedef struct pl_ctx pl_ctx;     /* one device + one stream + one memory pool */
typedef struct pl_graph pl_graph; /* a captured forward pass (hipGraphExec)     */
typedef struct pl_plan pl_plan;   /* a whole compiled forward pass read from a plan file (pl_plan_build) */
typedef struct pl_event pl_event; /* hipEvent on the context stream             */

/* ---- runtime --------------------------------------------------------- */
const char *pl_last_error(void);
int pl_version(void);
int pl_device_count(int *count);
int pl_ctx_create(int device, pl_ctx **out);
int pl_ctx_destroy(pl_ctx *ctx);
int pl_ctx_info(pl_ctx *ctx, int *device, int *cu_count, size_t *hbm_bytes,
                char *arch_name, size_t arch_name_len);
/* "domain:bus:device.function" of the context's GPU (what /sys/bus/pci/devices/ is keyed by): lets a host tool
 * read the card's clocks from sysfs without forking a management CLI. */
int pl_ctx_pci_bus_id(pl_ctx *ctx, char *bus_id, size_t len);
int pl_sync(pl_ctx *ctx); /* wait for the context stream */

/* memory: replaces numpy/cupy array allocation (np.zeros, util.py:31-32,88) */
int pl_alloc(pl_ctx *ctx, size_t bytes, void **out); /* pooled, stream-ordered */
int pl_free(pl_ctx *ctx, void *ptr);
int pl_pool_stats(pl_ctx *ctx, size_t *bytes_reserved, size_t *bytes_in_use);
int pl_pool_block(pl_ctx *ctx, const void *ptr, void **base, size_t *bytes); /* the pool block that holds ptr */
int pl_pool_trim(pl_ctx *ctx);                       /* hipFree cached blocks */
/* Hygiene mode of the pool, for tests (off by default).  While guard_bytes != 0 every pl_alloc outside capture, the library's
 * own workspaces included, gets a hipMalloc of its own laid out [front guard][payload of exactly the requested bytes][back
 * guard]; the guards hold a canary byte, the payload poison_byte (-1: not filled, else 0..255).  Such a block is never
 * recycled: pl_free keeps it until the next check.  pl_pool_debug_check waits for the stream, compares the guards of every
 * live hygiene block and of every one freed since the last check, releases the freed ones, and sets *violations to the
 * number of dirty blocks; `report` (may be NULL) names the first few: serial, requested bytes, live or freed, side, offsets
 * of the first and last dirty byte from the payload edge, dirty byte count.  guard_bytes 0 switches the mode off; blocks
 * made under it stay valid. */
int pl_pool_debug(pl_ctx *ctx, size_t guard_bytes, int poison_byte);
int pl_pool_debug_check(pl_ctx *ctx, int *violations, char *report, size_t report_len);
/* np.asarray / .get() of net.py:96-100 */
int pl_h2d(pl_ctx *ctx, void *dst, const void *src_host, size_t bytes);
int pl_d2h(pl_ctx *ctx, void *dst_host, const void *src, size_t bytes); /* syncs */
int pl_d2d(pl_ctx *ctx, void *dst, const void *src, size_t bytes);
int pl_memset(pl_ctx *ctx, void *dst, int byte, size_t bytes);
/* The asynchronous halves of the same contract (host ndarray in, host ndarray out: net.py:94-101).
 *   pl_h2d_staged  copies src_host into a ring of pinned buffers, chunk by chunk (library copy threads), and enqueues each
 *                  chunk's DMA on `consumer`'s stream (NULL: ctx's own) while the next is staged.  Returns as soon as
 *                  src_host has been read -- the caller may overwrite it -- and nothing waits for the bytes except what
 *                  `consumer` enqueues afterwards.  dst is a block of ctx's pool; the copy is ordered behind what ctx's stream
 *                  held at the call.  A src_host inside pl_host_alloc memory is NOT staged: the DMA reads it in place, later,
 *                  so the caller keeps it unchanged until `consumer`'s stream has passed the copy (a pl_event tells).
 *   pl_d2h_begin   enqueues device -> pinned buffer on `producer`'s stream (NULL: ctx's); *ticket identifies the buffer
 *                  (-1: every buffer is in flight, use pl_d2h).  No host wait.
 *   pl_d2h_finish  waits for that copy, moves the bytes to dst_host (NULL: drops them), releases the buffer.  The device
 *                  block must stay allocated until then.
 *   pl_host_alloc / pl_host_free   pinned host memory for callers that build batches in place.
 *   pl_copy_threads                worker threads of the staging copies (PLANER_HIP_COPY_THREADS; the caller's thread works too).
 * PLANER_HIP_COPY_STREAMS=1 moves the DMAs onto two dedicated copy streams (measured slower on MI355X: DESIGN 4.8). */
int pl_h2d_staged(pl_ctx *ctx, pl_ctx *consumer, void *dst, const void *src_host, size_t bytes);
/* host -> device at once and on NO stream: the host waits for the DMA, no hardware queue does.  The caller guarantees that no
 * work on the device still uses dst.  (What Net.submit feeds a pipeline's replicas with: DESIGN 4.8.) */
int pl_h2d_direct(pl_ctx *ctx, void *dst, const void *src_host, size_t bytes);
int pl_d2h_begin(pl_ctx *ctx, pl_ctx *producer, const void *src, size_t bytes, int *ticket);
int pl_d2h_finish(pl_ctx *ctx, int ticket, void *dst_host);
int pl_host_alloc(size_t bytes, void **out);
int pl_host_free(void *ptr);
int pl_copy_threads(int *workers);

/* timing: fills Net.timer (net.py:55,67-70) with device time */
int pl_event_create(pl_ctx *ctx, pl_event **out);
int pl_event_record(pl_ctx *ctx, pl_event *ev);
int pl_event_sync(pl_event *ev);        /* host waits until the recorded point of the stream has been reached */
int pl_event_elapsed_ms(pl_event *start, pl_event *stop, float *ms); /* syncs on stop */
int pl_event_destroy(pl_event *ev);

/* fork/join between two contexts (streams) of one device */
int pl_stream_wait(pl_ctx *waiter, pl_ctx *signal);
/* the waiter's stream waits for one recorded point of another stream (Net.submit: a pending result is handed to the
 * caller's stream without waiting for what was queued behind it) */
int pl_stream_wait_event(pl_ctx *waiter, pl_event *ev);
/* Exchange the streams of two idle contexts of one device (each keeps its memory pool, graphs and events).  Which hardware queue
 * a stream runs on is fixed when the runtime creates it; the plan compiler uses this to try assignments of pipeline replicas
 * to streams without re-capturing their graphs.  No counterpart in the reference (net.py has no notion of a stream). */
int pl_ctx_swap_streams(pl_ctx *a, pl_ctx *b);

/* whole-forward capture: the HIP-native replacement for interpreting the flow
 * in Python on every call (net.py:37-72).  Between begin/end every launch and
 * pool allocation on the context is recorded instead of executed. */
int pl_capture_begin(pl_ctx *ctx);
int pl_capture_end(pl_ctx *ctx, pl_graph **out);
int pl_graph_launch(pl_graph *g);
int pl_graph_destroy(pl_graph *g);

/* ---- a compiled forward pass without the Python host ----------------------------------------
 * Replaces the reference's interpreter loop (net.Net.forward, net.py:37-72) for hosts that bind this header directly.
 * A plan file (written once by planer_amd.export.export_plan from a loaded Net and an input shape) holds the FUSED program of
 * the plan compiler -- fused conv epilogues, channel-quad layouts, Winograd stages and chains, paired convs -- as the flat
 * sequence of calls of this ABI, with the constants (weights, prepared filters) and the activation arena's size.
 *   pl_plan_build    parses the file, uploads the constants, runs the sequence once and captures it into a hipGraph
 *   pl_plan_tensor   input / output i: the plan's own device buffer, its size, element type (0 f32, 1 i32, 2 i64, 3 u8) and shape
 *   pl_plan_run      copies inputs[i] (device pointers; NULL = the caller wrote the plan's buffer itself) in, launches the
 *                    graph, copies the outputs to outputs[i] (device pointers; NULL = read the plan's buffer) -- asynchronous
 *                    on the context's stream like every other call (pl_sync waits)
 *   pl_plan_destroy  frees graph, arena and constants */
int pl_plan_build(pl_ctx *ctx, const void *program, size_t program_bytes, pl_plan **out);
int pl_plan_info(pl_plan *plan, int *n_inputs, int *n_outputs, size_t *arena_bytes, size_t *const_bytes, int *n_calls);
int pl_plan_tensor(pl_plan *plan, int output, int index, void **device_ptr, size_t *bytes, int *dtype, int *ndim, int *dims8);
int pl_plan_run(pl_plan *plan, const void *const *inputs, void *const *outputs);
int pl_plan_destroy(pl_plan *plan);

/* ---- MFMA-bound ops --------------------------------------------------- */
/* layer.Conv2d (layer.py:22-26) == util.conv_for (util.py:17-44) + bias add.
 * Implicit-GEMM: (Cout x Cin/g*kh*kw) @ im2col(x), K ordered (cin,kh,kw) like
 * K.reshape(Cout,-1); output Ho = (H+pt+pb-(kh-1)*dh-1+sh)/sh (util.py:25-26).
 * Requires pt==pb and pl==pr (util.pad, util.py:8) else PL_EUNSUPPORTED.
 * bias may be NULL. */
int pl_conv2d_f32(pl_ctx *ctx, const float *x, int N, int Cin, int H, int W,
                  const float *w, int Cout, int kh, int kw, const float *bias,
                  float *y, int sh, int sw, int dh, int dw, int pt, int pl,
                  int pb, int pr, int group);

/* Conv2d with the layers that follow it folded into the epilogue, used by
 * the compiled plan:  y = act( (conv(x,w)+bias) * scale[c] + shift[c] + res )
 * i.e. conv -> batchnorm (layer.py:125-127) -> add (layer.py:93-95) ->
 * relu/leakyrelu (layer.py:44-51).  scale/shift/res/bias may each be NULL.
 * With act | PL_ACT_RES_AFTER:  y = act( (conv+bias)*scale + shift ) + res. */
int pl_conv2d_fused_f32(pl_ctx *ctx, const float *x, int N, int Cin, int H,
                        int W, const float *w, int Cout, int kh, int kw,
                        const float *bias, float *y, int sh, int sw, int dh,
                        int dw, int pt, int pl, int pb, int pr, int group,
                        const float *scale, const float *shift,
                        const float *res, int act, double alpha, int w_layout);

/* w_layout 0: filters exactly as the reference holds them, OIHW (layer.py:22).
 * w_layout 1: "tap-major" filters [Cout][kh*kw][Cin/g] produced once per model
 * by pl_conv2d_prepare_weights_f32 (needs Cin/g % 16 == 0); lets the kernel
 * compute padding validity once per K-chunk instead of once per element.
 * 1x1 filters are identical in both layouts. */
int pl_conv2d_prepare_weights_f32(pl_ctx *ctx, const float *w, int Cout, int Cin_g,
                                  int kh, int kw, float *out);
/* w_layout 3: Winograd F(2x2,3x3) filters U[16][Cout][Cin] (16*Cout*Cin floats) for 3x3 /
 * stride 1 / pad 1 / group 1 convs with Cin % 16 == 0: input transform + 16 GEMMs (one grouped
 * 1x1 conv on the MFMA kernel) + output transform with the fused tail. */
int pl_conv2d_prepare_winograd_f32(pl_ctx *ctx, const float *w, int Cout, int Cin, float *out);
/* ---- channel-quad ("Q4") activations: the compiled plan's internal layout ----
 * A Q4 tensor holds the reference's (N,C,H,W) array as [N][ceil(C/4)][H][W][4]
 * (channel c -> quad c/4, lane c%4; padding lanes are zero), 16-byte aligned.
 * It exists because on gfx950 one b128 load per (pixel, 4 channels) keeps the
 * fp32 MFMA pipe 13-17 % busier than the four dword loads NCHW needs (DESIGN.md
 * section 4).  Semantics stay layer.Conv2d's (layer.py:22-26, util.py:17-44):
 * pl_q4_to_nchw(pl_conv2d_q4(pl_nchw_to_q4(x))) == pl_conv2d_fused(x) up to
 * fp32 summation order.  Conversions are done by the plan at graph inputs /
 * outputs and around layers that have no Q4 kernel. */
int pl_nchw_to_q4_f32(pl_ctx *ctx, const float *x, float *yq, int N, int C, int HW);
int pl_q4_to_nchw_f32(pl_ctx *ctx, const float *xq, float *y, int N, int C, int HW);
/* Filter for pl_conv2d_q4_f32: OIHW -> wq[group][q][Cout/group][4] with
 * q = tap*ceil(Cin_g/4) + cin/4, zero padded to a multiple of 8 k-quads; made
 * once per model.  `elems` = floats the packed filter occupies. */
int pl_conv2d_q4_filter_elems(int Cout, int Cin_g, int kh, int kw, int group, size_t *elems);
int pl_conv2d_prepare_q4_f32(pl_ctx *ctx, const float *w, int Cout, int Cin_g, int kh, int kw,
                             int group, float *out);
/* pl_conv2d_fused_f32 on Q4 tensors: xq, resq, yq are Q4 (Cin / Cout / Cout
 * channels); bias/scale/shift stay plain per-channel arrays.  group > 1 needs
 * Cin/group and Cout/group to be multiples of 4 (else PL_EUNSUPPORTED). */
int pl_conv2d_q4_f32(pl_ctx *ctx, const float *xq, int N, int Cin, int H, int W,
                     const float *wq, int Cout, int kh, int kw, const float *bias,
                     float *yq, int sh, int sw, int dh, int dw, int pt, int pl,
                     int pb, int pr, int group, const float *scale,
                     const float *shift, const float *resq, int act, double alpha);

/* Depthwise convs (group == Cin == Cout, one filter plane per channel) on Q4 tensors: the fused
 * tail of pl_conv2d_q4_f32 on a VALU kernel that stages each output tile's input window in LDS
 * (any kh x kw, stride, dilation; symmetric pads).  pl_conv2d_fused_f32 takes the same kernel's
 * NCHW form by itself for w_layout 0.  wq ("w_layout 13") from pl_conv2d_prepare_dw_q4_f32:
 * OIHW [C][1][kh][kw] -> [ceil(C/4)][kh*kw][4], zero-padded quads: ceil(C/4)*kh*kw*4 floats. */
int pl_conv2d_prepare_dw_q4_f32(pl_ctx *ctx, const float *w, int C, int kh, int kw, float *out);
int pl_conv2d_dw_q4_f32(pl_ctx *ctx, const float *xq, int N, int C, int H, int W,
                        const float *wq, int kh, int kw, const float *bias, float *yq,
                        int sh, int sw, int dh, int dw, int pt, int pl, int pb, int pr,
                        const float *scale, const float *shift, const float *resq, int act,
                        double alpha);
/* Transposed convs (ConvTranspose2d, filter [Cin][Cout][kh][kw], group 1, dilation 1) on Q4 tensors, by output
 * phase: each of the sh*sw phases is a stride-1 conv of x with a ceil(kh/sh) x ceil(kw/sw) sub-filter, written to
 * every sh-th row / sw-th column of y -- no zero-stuffed input.  Output Ho = (H-1)*sh - pt - pb + kh + oph (Wo
 * alike); pads may be asymmetric up to the kernel reach (pt <= kh-1, pb <= kh-1+oph).  The fused tail is
 * pl_conv2d_q4_f32's.  wq ("w_layout 14") from pl_conv2d_prepare_convt_q4_f32: [sh*sw][q][Cout][4] with
 * q = tap*ceil(Cin/4) + cin/4 padded to a multiple of 8, pl_conv2d_convt_filter_elems floats. */
int pl_conv2d_convt_filter_elems(int Cin, int Cout, int kh, int kw, int sh, int sw, size_t *elems);
int pl_conv2d_prepare_convt_q4_f32(pl_ctx *ctx, const float *w, int Cin, int Cout, int kh, int kw,
                                   int sh, int sw, float *out);
int pl_conv2d_convt_q4_f32(pl_ctx *ctx, const float *xq, int N, int Cin, int H, int W,
                           const float *wq, int Cout, int kh, int kw, const float *bias, float *yq,
                           int sh, int sw, int dh, int dw, int pt, int pl, int pb, int pr, int oph,
                           int opw, const float *scale, const float *shift, const float *resq,
                           int act, double alpha);
/* Winograd F(2x2,3x3) on Q4 tensors for 3x3 / stride 1 / pad 1 / group 1 convs with
 * Cin % 4 == 0 and Cout % 4 == 0: uq = [16][k-quad][Cout][4] filters made once per
 * model; float4 input/output transforms around one grouped 1x1 Q4 conv. */
int pl_conv2d_winograd_q4_filter_elems(int Cout, int Cin, size_t *elems);
int pl_conv2d_prepare_winograd_q4_f32(pl_ctx *ctx, const float *w, int Cout, int Cin, float *out);
int pl_conv2d_winograd_q4_f32(pl_ctx *ctx, const float *xq, int N, int Cin, int H, int W,
                              const float *uq, int Cout, const float *bias, float *yq,
                              const float *scale, const float *shift, const float *resq,
                              int act, double alpha);

/* Row-packed convolution for inputs with 1..3 channels (the 7x7 / 3-channel stem): takes the
 * reference's NCHW input directly, re-lays it as a zero-padded NHWC image (one HBM pass, replaces
 * pl_nchw_to_q4_f32 for this layer) and runs conv_q4_kernel with K = kh rows x ceil(kw*Cin/4)
 * quads instead of kh*kw taps x 1 padded quad (7x7x3: 168 instead of 196 k-values, no range checks
 * in the gather).  wq from pl_conv2d_prepare_rowpack_f32; output and residual are Q4.
 * group 1, dilation 1, symmetric pads. */
int pl_conv2d_rowpack_filter_elems(int Cout, int Cin, int kh, int kw, size_t *elems);
int pl_conv2d_prepare_rowpack_f32(pl_ctx *ctx, const float *w, int Cout, int Cin, int kh, int kw,
                                  float *out);
int pl_conv2d_rowpack_q4_f32(pl_ctx *ctx, const float *x, int N, int Cin, int H, int W,
                             const float *wq, int Cout, int kh, int kw, const float *bias,
                             float *yq, int sh, int sw, int pt, int pl, const float *scale,
                             const float *shift, const float *resq, int act, double alpha);
/* The two halves of pl_conv2d_rowpack_q4_f32, for callers that own the input buffer of a captured plan: the re-layout
 * (x NCHW -> xp, pl_rowpack_input_elems floats, 16-byte aligned) can then BE the copy that brings a new batch into the
 * plan -- planer_amd.net feeds a plan this way instead of copying the batch and re-laying it inside the graph -- and the
 * convolution reads the packed image.  Same kernels, same results as the one-call form (util.py:17-44). */
int pl_rowpack_input_elems(int N, int Cin, int H, int W, int kw, int sw, int pt, int pl, size_t *elems);
int pl_rowpack_input_f32(pl_ctx *ctx, const float *x, float *xp, int N, int Cin, int H, int W, int kw,
                         int sw, int pt, int pl);
int pl_conv2d_rowpacked_q4_f32(pl_ctx *ctx, const float *xp, int N, int Cin, int H, int W,
                               const float *wq, int Cout, int kh, int kw, const float *bias,
                               float *yq, int sh, int sw, int pt, int pl, const float *scale,
                               const float *shift, const float *resq, int act, double alpha);
/* The row-packed stem conv FOLLOWED BY layer.Maxpool(w = 3x3, strides 2, pads 1) (layer.py:71-72 -> util.pool util.py:79-95:
 * zero padding, running maximum from -1e4) in one kernel that writes only the pooled Q4 tensor [N][Cout/4][Hq][Wq][4]
 * (conv_stem_pool_kernel.h: a persistent workgroup marches down an image strip, conv rows live in LDS only).  Built for the
 * stem of an ImageNet-style net -- 3 channels, 7x7 / stride 2 / pad 3, input width 224; _supported says whether a shape
 * qualifies, anything else is PL_EUNSUPPORTED (the plan compiler then keeps the two kernels).  bias / scale / shift are
 * read as 16-byte channel quads; no residual. */
int pl_conv2d_rowpacked_pool_supported(int Cin, int H, int W, int Cout, int kh, int kw, int sh, int sw, int pt,
                                       int pl, int *ok);
int pl_conv2d_rowpacked_pool_q4_f32(pl_ctx *ctx, const float *xp, int N, int Cin, int H, int W,
                                    const float *wq, int Cout, int kh, int kw, const float *bias,
                                    float *yq, int sh, int sw, int pt, int pl, const float *scale,
                                    const float *shift, int act, double alpha);
/* The same kernel reading the reference's NCHW input itself (no row-packed copy of the batch; util.conv_for util.py:17-44 gathers
 * from the padded NCHW tensor too): 3 channels, 7x7 / stride 2 / pad 3, W % 4 == 0, x 16-byte aligned.  wq = the filter in this
 * kernel's k order, [48][Cout][4] floats (_filter_elems) made by pl_conv2d_prepare_stem_nchw_f32 from OIHW [Cout][3][7][7].
 * strip_rows: pooled rows per workgroup strip -- 0 or 7 (one workgroup per CU at batch 32 / 224 px), or 14: half the workgroups
 * running 15 instead of 2 x 8 conv-row pairs, slower alone and cheaper for a pipelined host. */
int pl_conv2d_stem_pool_nchw_supported(int Cin, int H, int W, int Cout, int kh, int kw, int sh, int sw, int pt,
                                       int pl, int *ok);
int pl_conv2d_stem_nchw_filter_elems(int Cout, size_t *elems);
/* The k order of that filter (host query, no device): tab[4 q + j] = 8 rho + kw + 1 for element j of k-quad q, rho = 3 * filter
 * row + channel, kw = -1 a zero filter value; -1 where the slot holds no tap.  37 quads (K = 148): n >= 148. */
int pl_conv2d_stem_nchw_korder(int *tab, int n);
int pl_conv2d_prepare_stem_nchw_f32(pl_ctx *ctx, const float *w, int Cout, float *out);
int pl_conv2d_stem_pool_nchw_q4_f32(pl_ctx *ctx, const float *x, int N, int H, int W, const float *wq, int Cout,
                                    const float *bias, float *yq, const float *scale, const float *shift,
                                    int act, double alpha, int strip_rows);
/* A second form of that kernel: a polyphase 1-D Winograd F(4,4) along W (conv_stem_wino_kernel.h; nodes 0, 1, -1, 2, -2, 1/2,
 * inf) -- 7 frequency GEMMs of K = 44 instead of one of K = 148.  Same shapes and arguments; wq = G g in that kernel's k order,
 * [7][11][Cout][4] floats, made by pl_conv2d_prepare_stem_wino_f32 from OIHW [Cout][3][7][7].  Not bit-exact on integers.
 * _korder: tab[4 k + a] = index into one output channel's [3][7][7] filter of tap a of k (element e of quad q is k = 4 q + e), or
 * -1 for a zero; n >= 176. */
int pl_conv2d_stem_pool_wino_supported(int Cin, int H, int W, int Cout, int kh, int kw, int sh, int sw, int pt,
                                       int pl, int *ok);
int pl_conv2d_stem_wino_filter_elems(int Cout, size_t *elems);
int pl_conv2d_stem_wino_korder(int *tab, int n);
int pl_conv2d_prepare_stem_wino_f32(pl_ctx *ctx, const float *w, int Cout, float *out);
int pl_conv2d_stem_pool_wino_q4_f32(pl_ctx *ctx, const float *x, int N, int H, int W, const float *wq, int Cout,
                                    const float *bias, float *yq, const float *scale, const float *shift,
                                    int act, double alpha, int strip_rows);
/* Winograd F(4x4,3x3) on Q4 tensors (same constraints as the F(2x2,3x3) entry points): 6x6 input
 * tiles, 36 grouped GEMMs, 4x fewer multiplies than the direct conv and less transform traffic
 * than F(2x2,3x3); larger transform constants, error a few 1e-6 of max|y| in fp32.
 * uq = [36][k-quad][Cout][4]. */
int pl_conv2d_winograd4_q4_filter_elems(int Cout, int Cin, size_t *elems);
int pl_conv2d_prepare_winograd4_q4_f32(pl_ctx *ctx, const float *w, int Cout, int Cin, float *out);
int pl_conv2d_winograd4_q4_f32(pl_ctx *ctx, const float *xq, int N, int Cin, int H, int W,
                               const float *uq, int Cout, const float *bias, float *yq,
                               const float *scale, const float *shift, const float *resq,
                               int act, double alpha);

/* The same F(4x4,3x3) pipeline stage by stage, for plans that chain consecutive Winograd convs
 * (replaces util.conv_for, util.py:17-44, for 3x3 / stride 1 / pad 1 convs; the fused tail is
 * layer.BatchNorm / Add / ReLU / LeakyReLU, layer.py:125-127, 93-95, 44-51).
 * V (transformed input) and M (per-frequency products) are [36][C/4][T][4] with
 * T = N * ceil(H/4) * ceil(W/4); pl_wino4_elems gives their size in floats.
 *   pl_wino4_input_q4_f32    xq (N,C,H,W) -> V
 *   pl_wino4_gemm_q4_f32     V (Cin), uq (prepare_winograd4) -> M (Cout): 36 grouped GEMMs on the MFMA kernel
 *   pl_wino4_output_q4_f32   M -> yq = act((A^T m A + bias)*scale + shift + res)
 *   pl_wino4_chain_q4_f32    M -> yq (may be NULL: nobody else reads it) AND Vnext, the transformed input of
 *                            the next 3x3 conv on yq, in one kernel: yq never makes the round trip through HBM
 * pl_wino4_chain_supported: *ok = 1 when an (N,C,H,W) map fits the LDS transform kernel (whole planes per
 * workgroup); otherwise pl_wino4_chain_q4_f32 returns PL_EUNSUPPORTED and input / output use the register
 * kernels.  Results are bit-identical to pl_conv2d_winograd4_q4_f32 whichever kernels run. */
int pl_wino4_elems(int N, int C, int H, int W, size_t *elems);
int pl_wino4_chain_supported(pl_ctx *ctx, int N, int C, int H, int W, int *ok);
int pl_wino4_input_q4_f32(pl_ctx *ctx, const float *xq, int N, int C, int H, int W, float *V);
int pl_wino4_gemm_q4_f32(pl_ctx *ctx, const float *V, int N, int Cin, int H, int W, const float *uq, int Cout, float *M);
int pl_wino4_output_q4_f32(pl_ctx *ctx, const float *M, int N, int C, int H, int W, const float *bias,
                           const float *scale, const float *shift, const float *resq, int act, double alpha,
                           float *yq);
int pl_wino4_chain_q4_f32(pl_ctx *ctx, const float *M, int N, int C, int H, int W, const float *bias,
                          const float *scale, const float *shift, const float *resq, int act, double alpha,
                          float *yq, float *Vnext);

/* Winograd with MIXED tiles for maps whose sides are 7, 14 or 21 pixels (csrc/wino43_kernels.h): a side of 7a is cut into a
 * segments of 4 (F(4,3), 6 frequencies) and a segments of 3 (F(3,3), 5 frequencies), so no tile hangs over the map's edge --
 * F(4x4,3x3) computes a 14x14 map as 16x16 and a 7x7 map as 8x8.  Four tile classes (6x6, 6x5, 5x6, 5x5 frequencies) with equally
 * many tiles each: 121 per-frequency GEMMs of N a^2 columns, one grouped launch.  Same contract as the pl_wino4_* stages /
 * pl_conv2d_winograd4_q4_f32 (3x3 / stride 1 / pad 1 / group 1, Cin and Cout multiples of 4, fused tail); V / M are
 * [121][C/4][N (H/7) (W/7)][4]; replaces the same reference code (layer.py:22-26 -> util.py:17-44). */
int pl_wino43_supported(int H, int W, int *ok);
int pl_wino43_elems(int N, int C, int H, int W, size_t *elems);
int pl_conv2d_winograd43_q4_filter_elems(int Cout, int Cin, size_t *elems);
int pl_conv2d_prepare_winograd43_q4_f32(pl_ctx *ctx, const float *w, int Cout, int Cin, float *out);
int pl_wino43_input_q4_f32(pl_ctx *ctx, const float *xq, int N, int C, int H, int W, float *V);
int pl_wino43_gemm_q4_f32(pl_ctx *ctx, const float *V, int N, int Cin, int H, int W, const float *uq, int Cout, float *M);
int pl_wino43_output_q4_f32(pl_ctx *ctx, const float *M, int N, int C, int H, int W, const float *bias, const float *scale,
                            const float *shift, const float *resq, int act, double alpha, float *yq);
int pl_wino43_chain_q4_f32(pl_ctx *ctx, const float *M, int N, int C, int H, int W, const float *bias, const float *scale,
                           const float *shift, const float *resq, int act, double alpha, float *yq, float *Vnext);
int pl_conv2d_winograd43_q4_f32(pl_ctx *ctx, const float *xq, int N, int Cin, int H, int W, const float *uq, int Cout,
                                const float *bias, float *yq, const float *scale, const float *shift, const float *resq,
                                int act, double alpha);

/* A 1x1 / stride 1 / group 1 channel-quad convolution with its fused tail (bias, scale, shift, ReLU / LeakyReLU; no residual)
 * whose only reader is a staged Winograd 3x3 convolution: writes that conv's transformed input V straight away --
 * wino = 4: F(4x4,3x3), V as pl_wino4_input_q4_f32 makes it (wino = 2, the F(2x2,3x3) domain, is reserved: PL_EUNSUPPORTED).
 * wq from pl_conv2d_prepare_q4_f32 (group 1).  Replaces, for a Darknet block (1x1 then 3x3), layer.Conv2d + BatchNorm +
 * LeakyReLU (reference layer.py:22-26, 125-127, 48-51) and the first stage of the next conv; plan-internal. */
int pl_conv1x1_wino_in_q4_f32(pl_ctx *ctx, const float *xq, int N, int Cin, int H, int W, const float *wq, int Cout,
                              const float *bias, const float *scale, const float *shift, int act, double alpha, int wino,
                              float *V);

/* Two channel-quad convolutions that read the SAME input, in one launch (both with the fused tail
 * y = act((conv + bias) * scale + shift), no residual; group 1, dilation 1, symmetric pads; filters from
 * pl_conv2d_prepare_q4_f32).  Replaces two calls of util.conv_for (util.py:17-44) where a graph forks: ResNet's
 * stride-2 3x3 conv and the 1x1 stride-2 projection beside it -- the projection's tiles fill the tail of the
 * sibling's grid and find the pixels it gathers in the L2.  Results equal the two separate launches bit for bit
 * when those run unsplit with the same tile configuration. */
int pl_conv2d_q4_pair_f32(pl_ctx *ctx, const float *xq, int N, int Cin, int H, int W,
                          const float *wq_a, int Cout_a, int kh_a, int kw_a, int sh_a, int sw_a, int pt_a, int pl_a,
                          const float *bias_a, const float *scale_a, const float *shift_a, int act_a, double alpha_a, float *yq_a,
                          const float *wq_b, int Cout_b, int kh_b, int kw_b, int sh_b, int sw_b, int pt_b, int pl_b,
                          const float *bias_b, const float *scale_b, const float *shift_b, int act_b, double alpha_b, float *yq_b);

/* Fully fused Winograd F(4x4,3x3) on Q4 tensors (3x3 / stride 1 / pad 1 / group 1, Cin %% 4 == 0, Cout %% 4 == 0;
 * replaces util.conv_for, util.py:17-44, + the fused tail): one workgroup carries 32 tiles x 64 output channels
 * through all 36 frequencies -- input transform into LDS, v_mfma_f32_16x16x4_f32 with the 36 accumulator blocks in
 * registers, lane-local output transform -- so neither the transformed input nor the products ever reach memory.
 * u = filters laid out [Cout/64][Cin/4][36][4][4][16] by pl_conv2d_prepare_wf4_f32.  bias / scale / shift must be
 * 16-byte aligned (read as one 16-byte load per channel quad). */
int pl_conv2d_wf4_filter_elems(int Cout, int Cin, size_t *elems);
int pl_conv2d_prepare_wf4_f32(pl_ctx *ctx, const float *w, int Cout, int Cin, float *out);
int pl_conv2d_wf4_q4_f32(pl_ctx *ctx, const float *xq, int N, int Cin, int H, int W,
                         const float *u, int Cout, const float *bias, float *yq,
                         const float *scale, const float *shift, const float *resq,
                         int act, double alpha);

/* Fused 1-D Winograd F(4,3) along W on Q4 tensors (3x3 / stride 1 / pad 1 / group 1, Cin %% 4 == 0): 6 frequencies,
 * 4 outputs per tile, 2x fewer multiplies than the direct conv with NO extra HBM traffic -- the input transform happens
 * between the global load and LDS, the output transform in registers (conv_w1d_kernel.h).
 * uq = [6][k-quad][Cout][4], k-quad = row*Cin/4 + cin/4, made once per model. */
int pl_conv2d_w1d4_q4_filter_elems(int Cout, int Cin, size_t *elems);
int pl_conv2d_prepare_w1d4_q4_f32(pl_ctx *ctx, const float *w, int Cout, int Cin, float *out);
int pl_conv2d_w1d4_q4_f32(pl_ctx *ctx, const float *xq, int N, int Cin, int H, int W,
                          const float *uq, int Cout, const float *bias, float *yq,
                          const float *scale, const float *shift, const float *resq,
                          int act, double alpha);

/* HBM-bound layers on Q4 tensors (same semantics as their NCHW namesakes below:
 * util.pool util.py:79-92, layer.UpSample layer.py:80-82, layer.GlobalAveragePool
 * layer.py:77-78, layer.BatchNorm layer.py:125-127).  pl_gap_q4_f32 writes a
 * plain [N][C] array.  Element-wise layers (relu, leakyrelu, add ...) are layout
 * agnostic and run the ordinary kernels on the padded buffer. */
int pl_pool2d_q4_f32(pl_ctx *ctx, const float *xq, float *yq, int N, int C, int H, int W,
                     int kh, int kw, int sh, int sw, int pt, int pl, int pb, int pr,
                     int mode);
int pl_upsample_nearest_q4_f32(pl_ctx *ctx, const float *xq, float *yq, int N, int C,
                               int H, int W, int fh, int fw);
/* The channel-quad twins of pl_upsample_linear_f32 / pl_resize_linear_f32 (below): same host weight table and same device
 * position tables, per component the same roundings, so from_q4(twin(to_q4(x))) equals the NCHW entry bit for bit.  `resq`: NULL
 * or a Q4 tensor of the output's shape, added in the write pass as a rounding of its own (= the upsample followed by pl_add_f32).
 * Every quad of yq is written; xq != yq; fewer than 2^30 output quads. */
int pl_upsample_linear_q4_f32(pl_ctx *ctx, const float *xq, float *yq, const float *resq, int N, int C, int H, int W, int fh,
                              int fw, const float *weights);
int pl_resize_linear_q4_f32(pl_ctx *ctx, const float *xq, float *yq, const float *resq, int N, int C, int H, int W, int OH,
                            int OW, const int *ra, const float *rs, const int *ca, const float *cs);
/* layer.Concatenate (axis 1) of two Q4 tensors in one launch; the first is nearest-upsampled by (fh, fw) on the way
 * (layer.UpSample + layer.Concatenate, layer.py:80-82, 90-91): a is (N, Ca, H/fh, W/fw), b (N, Cb, H, W), y (N, Ca+Cb, H, W). */
int pl_concat2_q4_f32(pl_ctx *ctx, const float *aq, const float *bq, float *yq, int N, int Ca, int Cb, int H, int W, int fh,
                      int fw);
int pl_gap_q4_f32(pl_ctx *ctx, const float *xq, float *y, int N, int C, int HW);
int pl_scale_shift_q4_f32(pl_ctx *ctx, const float *xq, float *yq, const float *scale,
                          const float *shift, int N, int C, int HW);
/* layer.InstanceNormalization (layer.py:217-226) on a Q4 tensor IN PLACE with its tail fused into the write pass:
 * x = IN(x) [+ resq] [relu] (act 0 / 1), statistics per (image, channel), variance in the reference's centred form.
 * Planes of up to PL_INSTNORM_Q4_ONE_WG_PIXELS pixels are held by one workgroup per (image, quad): one read, one write.
 * Larger planes: chunks of PL_INSTNORM_Q4_CHUNK_PIXELS pixels give (mean, M2) partials in a pool block, merged in chunk order
 * (Chan's update) by the kernel that applies the tail.  The form depends on HW alone and there are no atomics: an image's bits
 * do not depend on the batch, nor on the run.  Padding lanes of a partial last quad are written as +0.0.  HW == 0 or
 * N == 0: nothing to do.  More than 2^29 quads: PL_EUNSUPPORTED. */
#define PL_INSTNORM_Q4_ONE_WG_PIXELS 4096
#define PL_INSTNORM_Q4_CHUNK_PIXELS 2048
int pl_instancenorm_q4_f32(pl_ctx *ctx, float *xq, const float *scale, const float *bias, const float *resq,
                           int N, int C, int HW, double eps, int act);
/* Group normalisation of a Q4 tensor IN PLACE, as the five steps an exporter writes for it (reshape to (N, G, -1),
 * InstanceNormalization with the G values gscale / gbias, reshape back, mul by gamma, add beta) with the tail in the
 * write pass: x = IN_g(x) [* gamma] [+ beta] [+ resq] [relu].  gamma, beta (C values each) and resq may be null; every operation
 * is rounded on its own, in that order.  Statistics per (image, group) in the centred form, no atomics.  The form depends on
 * cpg = C / G and HW alone: cpg % 4 == 0 (a group is one run of cpg / 4 * HW float4s), cpg == 2 (two groups per quad) or
 * cpg == 1 (the instance norm's geometry); runs / planes of up to PL_INSTNORM_Q4_ONE_WG_PIXELS float4s are held by one workgroup,
 * longer ones go through chunk partials merged in chunk order.  Padding lanes of a partial last quad are written as +0.0.
 * Any other cpg (3, 6, 10, ...) or more than 2^29 quads: PL_EUNSUPPORTED, before any launch.  C % G != 0: PL_EINVAL. */
int pl_groupnorm_q4_f32(pl_ctx *ctx, float *xq, const float *gscale, const float *gbias, const float *gamma, const float *beta,
                        const float *resq, int N, int C, int HW, int G, double eps, int act);
/* Pixel-phase re-layout of a Q4 tensor.  The (N, C, H, W) activation "folded by (dh, dw)" is the Q4
 * tensor of logical shape (N*dh*dw, C, ceil(H/dh), ceil(W/dw)): image (n*dh + i)*dw + j holds at pixel (r, c) the quads of
 * x[n, :, r*dh + i, c*dw + j], and zero in all four lanes where that coordinate lies outside H x W.  A 3x3 / stride 1 conv with
 * dilation (dh, dw) and pads (dh, dw, dh, dw) on x is the 3x3 / pad 1 / dilation 1 conv on the folded tensor.  This entry takes
 * a tensor folded by (dh_in, dw_in) to the same activation folded by (dh_out, dw_out); (1, 1) is the unfolded tensor, so it
 * folds, unfolds and goes from fold to fold.  N, C, H, W are the UNFOLDED shape.  Every output quad is written, the zero-fill
 * cells included; the input's zero-fill cells are never read (a conv leaves junk there).  Bits are moved, not computed on.
 * 2^29 quads or more on either side: PL_EUNSUPPORTED. */
int pl_refold_q4_f32(pl_ctx *ctx, const float *xq, float *yq, int N, int C, int H, int W, int dh_in, int dw_in, int dh_out,
                     int dw_out);

/* Pixel shuffle / unshuffle (depth-to-space / space-to-depth) of a Q4 tensor in one pass.  N, C, H, W describe the
 * NARROW side -- the output of a shuffle (inverse = 0), the input of an unshuffle (inverse = 1); the other side is the Q4 tensor
 * (N, C r^2, H / r, W / r).  order 0, CRD (PyTorch PixelShuffle / PixelUnshuffle): wide channel c r^2 + i r + j <-> narrow channel
 * c at pixel (h r + i, w r + j), any C.  order 1, DCR (ONNX DepthToSpace / SpaceToDepth): wide channel (i r + j) C + c, C % 4 == 0
 * only.  r = 2, 3, 4.  nchw_out (shuffles only): y is the plain (N, C, H, W) tensor instead of a Q4 one.  Every lane of a Q4
 * output is written, padding lanes as +0 whatever the input's hold; wide quads past ceil(C r^2 / 4) do not exist and are never
 * touched.  Bits are moved, not computed on.  xq != y, both 16-byte aligned; 2^29 quads or more on either side, another r, or DCR
 * with C % 4 != 0: PL_EUNSUPPORTED. */
int pl_pixel_shuffle_q4_f32(pl_ctx *ctx, const float *xq, float *y, int N, int C, int H, int W, int r, int order, int inverse,
                            int nchw_out);

/* First call for a new conv shape times every applicable tile configuration
 * and remembers the fastest (on by default; PLANER_HIP_AUTOTUNE=0 or 0 here
 * selects the static heuristic). Never runs during graph capture. */
int pl_set_autotune(pl_ctx *ctx, int enabled);
/* Persist / restore the tuned plans of a context (text file). */
int pl_tune_cache_save(pl_ctx *ctx, const char *path);
int pl_tune_cache_load(pl_ctx *ctx, const char *path, int *entries);
/* Force one tile configuration for the conv kernel (tuning / tests).
 * cfg < 0 restores the built-in heuristic. split_k <= 0 means automatic. */
int pl_conv2d_set_config(pl_ctx *ctx, int cfg, int split_k);
/* Full launch plan: tiles [0,dp_tiles) run data-parallel with the fused epilogue,
 * the rest as split_k slices + tile reduce; occupancy>0 pins workgroups per CU. */
int pl_conv2d_set_plan(pl_ctx *ctx, int cfg, int dp_tiles, int split_k, int occupancy);
int pl_conv2d_num_configs(void);
/* How the last convolution enqueued on this context was launched -- kernel family, tile
 * configuration, data-parallel tiles / split-K slices / occupancy pin, e.g.
 * "wino4[q64x64x16 dp=1800 split=1 occ=0]".  For run reports (bench.py config.algos). */
int pl_conv2d_last_plan(pl_ctx *ctx, char *buf, size_t len);
/* The GEMM that launch executed on the matrix cores, padding included: ext4 = {groups (Winograd: frequencies),
 * rows, columns, K} with rows / columns rounded up to whole tiles and K to whole chunks; executed FLOPs =
 * 2 * ext4[0] * ext4[1] * ext4[2] * ext4[3] (bench.py roofline.frac). */
int pl_conv2d_last_extents(pl_ctx *ctx, long long *ext4);
/* Launch-plan cache of this context's device: entries held, and how many conv shapes had to be timed
 * (autotuned) by this context because no entry existed (0 = every launch plan came from a loaded cache). */
int pl_tune_stats(pl_ctx *ctx, int *entries, int *misses);
int pl_conv2d_config_name(int cfg, char *buf, size_t len);

/* layer.Dense (layer.py:15-18): y[M,N] = x[M,K] @ w[N,K]^T + bias[N]  (trans_b=1)
 * layer.MatMul (layer.py:20):   y[M,N] = a[M,K] @ b[K,N]              (trans_b=0) */
int pl_gemm_f32(pl_ctx *ctx, const float *a, int M, int K, const float *b,
                int N, int trans_b, const float *bias, float *y);

/* ---- HBM-bound ops ----------------------------------------------------- */
/* layer.BatchNorm (layer.py:125-127): y = x*scale[c] + shift[c], x (outer,C,inner) */
int pl_scale_shift_f32(pl_ctx *ctx, const float *x, float *y, const float *scale,
                       const float *shift, int outer, int C, int inner);
/* layer.ReLU (layer.py:44-46): y = x*(x>0); the reference works in place (y==x) */
int pl_relu_f32(pl_ctx *ctx, const float *x, float *y, size_t n);
/* layer.LeakyReLU (layer.py:48-51): y = x*((x>0)*(1-alpha)+alpha) */
int pl_leakyrelu_f32(pl_ctx *ctx, const float *x, float *y, size_t n, double alpha);
/* layer.Sigmoid (layer.py:61-64): y = 1/(1+exp(-x)) */
int pl_sigmoid_f32(pl_ctx *ctx, const float *x, float *y, size_t n);
/* layer.Add (layer.py:93-95), same-shape and per-channel-broadcast forms */
int pl_add_f32(pl_ctx *ctx, const float *a, const float *b, float *y, size_t n);
int pl_add_channel_f32(pl_ctx *ctx, const float *a, const float *b_c, float *y,
                       int outer, int C, int inner);
/* layer.Maxpool / AveragePool (layer.py:71-75) -> util.pool (util.py:79-100):
 * zero padding, max accumulator initialised to -1e4; avg divides by kh*kw.
 * mode 0 = max, 1 = average. pads must be symmetric. */
int pl_pool2d_f32(pl_ctx *ctx, const float *x, float *y, int NC, int H, int W,
                  int kh, int kw, int sh, int sw, int pt, int pl, int pb, int pr,
                  int mode);
/* layer.UpSample nearest (layer.py:80-82, util.py:184-192): block replication */
int pl_upsample_nearest_f32(pl_ctx *ctx, const float *x, float *y, int NC, int H,
                            int W, int fh, int fw);
/* layer.Concatenate (layer.py:90-91) building block: copy `rows` rows of
 * `width` floats from src (row pitch src_pitch) to dst (row pitch dst_pitch) */
int pl_copy2d_f32(pl_ctx *ctx, float *dst, size_t dst_pitch, const float *src,
                  size_t src_pitch, size_t width, size_t rows);
/* layer.GlobalAveragePool (layer.py:77-78): y[r] = mean(x[r, 0:inner]) */
int pl_gap_f32(pl_ctx *ctx, const float *x, float *y, int rows, int inner);
/* ---- second-wave operators ---------------------------------- */
/* Exp/Log/Tanh/Sqrt/Reciprocal/HardSigmoid/Clip (layer.py:53,66-69,174-186,247-251).
 * op: 0 exp, 1 log, 2 tanh, 3 sqrt, 4 reciprocal, 5 hardsigmoid (p0=alpha,p1=beta),
 * 6 clip (p0=min,p1=max).  y may alias x (Clip works in place in the reference). */
int pl_unary_f32(pl_ctx *ctx, const float *x, float *y, size_t n, int op, double p0, double p1);
/* Add/Sub/Mul/Div/Pow (layer.py:93-111) on a result viewed as (outer,C,inner).
 * op: 0 add, 1 sub, 2 mul, 3 div, 4 pow.  a_mode/b_mode: 0 full-size operand,
 * 1 one value per channel (C), 2 a single value. */
int pl_binary_f32(pl_ctx *ctx, const float *a, const float *b, float *y, int outer, int C,
                  int inner, int op, int a_mode, int b_mode);
/* Add/Sub/Mul/Div/Pow under general numpy broadcasting (layer.py:93-111): `shape` is the
 * broadcast result (1..6 axes), a_stride / b_stride the operands' element strides per
 * result axis, 0 where the operand is broadcast.  op as in pl_binary_f32. */
int pl_binary_bcast_f32(pl_ctx *ctx, const float *a, const float *b, float *y, int ndim,
                        const int *shape, const long long *a_stride, const long long *b_stride,
                        int op);
/* layer.UpSample / Resize, mode "linear", integer factors (util.py:121-153
 * make_upmat + upsample_blinear): `weights` is a HOST table of terms x fh x fw floats
 * (terms = 4 when both factors exceed 1: lt, rt, lb, rb; else 2), fh * fw <= 64. */
int pl_upsample_linear_f32(pl_ctx *ctx, const float *x, float *y, int NC, int H, int W, int fh,
                           int fw, const float *weights);
/* layer.UpSample / Resize, mode "linear", fractional factors (util.py:194-219
 * upsample_size) on (NC, H, W) planes: ra/ca = lower sample row / column per output
 * row / column, rs/cs = the fractions (device arrays), columns first then rows. */
int pl_resize_linear_f32(pl_ctx *ctx, const float *x, float *y, int NC, int H, int W, int OH,
                         int OW, const int *ra, const float *rs, const int *ca, const float *cs);
/* Softmax / LogSoftmax over the last axis (layer.py:141-153) */
int pl_softmax_f32(pl_ctx *ctx, const float *x, float *y, int rows, int cols, int log_softmax);
/* ReduceSum/Mean/Max/Min over the trailing `cols` elements (layer.py:113-123): op 0..3 */
int pl_reduce_f32(pl_ctx *ctx, const float *x, float *y, int rows, int cols, int op);
/* Transpose (layer.py:194): y = x.transpose(perm), up to 6 axes */
int pl_transpose_f32(pl_ctx *ctx, const float *x, float *y, int ndim, const int *shape, const int *perm);
/* General strided map, up to 6 axes: output index o_d reads input index
 * t = o_d*step[d] + start[d] (wrap[d] = 1: taken modulo extent[d], 2: clamped to the
 * axis, 3 / 4: mirrored at its borders without / with the border sample -- np.pad's
 * 'wrap', 'edge', 'reflect', 'symmetric'; div[d] > 1: only
 * where t %% div[d] == 0, then t / div[d]) at in_stride[d] elements per index,
 * and `fill` wherever an axis falls outside [0, extent[d]).  Serves layer.Slice
 * (layer.py:188-196), layer.Pad in those five modes (:241-245), Tile (:57), Expand
 * (:198-200), Split (:170-172) and the zero-stuffing + filter flip/transpose of
 * layer.ConvTranspose2d (:28-34). */
int pl_strided_map_f32(pl_ctx *ctx, const float *x, float *y, int ndim, const int *out_shape,
                       const long long *in_stride, const int *start, const int *step,
                       const int *div, const int *extent, const int *wrap, double fill);
/* ---- operators of ONNX-exported detection heads (layer.py:155-157, 200-234, 253-258) -------------
 * pl_compare_f32: layer.Equal / Greater / GreaterOrEqual (op 0 / 1 / 2) -> bool bytes; *_one: that operand is one value.
 * pl_where_f32:   layer.Where, np.where(mask, a, b) with bool-byte mask.
 * pl_cast:        layer.Cast between 0 float32, 1 int32, 2 int64, 3 bool (numpy astype: truncation, != 0).
 * pl_gather_f32:  layer.Gather, np.take(x, idx, axis) on x viewed (outer, axis_len, inner); idx int32, negatives wrap.
 * pl_erf_lut_f32: layer.Erf -- clamps x IN PLACE like the reference and looks y up in its 1025-entry table `lut`.
 * pl_instancenorm_f32: layer.InstanceNormalization on (rows = N*C, inner) IN PLACE, scale/bias per channel.
 * pl_scatter_rows_f32: the device side of layer.Scatternd (layer.py:208-212): dst row dst_row[j] (rows of
 *                 row_len floats) = src row src_row[j]; the caller resolves index tuples to rows and keeps
 *                 only the last write to each row (the reference applies updates in order).
 * pl_nonzero_count / pl_nonzero_write: layer.NonZero (layer.py:230) = np.array(np.nonzero(x)) in two steps,
 *                 because the result's shape depends on the data: _count fills `scratch`
 *                 (ceil(n / PL_NONZERO_BLOCK) + 1 int64, device) and returns the number of non-zero elements in
 *                 *total (host; SYNCHRONISES the stream); _write fills out (ndim x total, int64, row-major
 *                 coordinates in ascending flat order).  elem_type as pl_cast.
 * pl_topk_f32:    layer.TopK (layer.py:234-239) on x viewed (outer, n, inner) along the middle axis: values /
 *                 int64 indices (outer, k, inner).  largest = 1: the k greatest, descending; largest = 0: k
 *                 copies of the smallest (the reference's index list is arange(k)*0).  NaN sorts last like
 *                 numpy; ties by ascending index (numpy leaves them unspecified).
 * pl_lstm_cell_f32: one time step of util.lstm (util.py:109-118) after the GEMMs: gates_x = x_t W^T,
 *                 gates_h = h R^T, both (N, 4H) in ONNX i|o|f|c order, bias (8H) = Wb | Rb; writes h, c (N, H). */
#define PL_NONZERO_BLOCK 2048
int pl_compare_f32(pl_ctx *ctx, const float *a, const float *b, unsigned char *y, size_t n, int op, int a_one, int b_one);
int pl_where_f32(pl_ctx *ctx, const unsigned char *mask, const float *a, const float *b, float *y, size_t n,
                 int a_one, int b_one);
int pl_cast(pl_ctx *ctx, const void *src, void *dst, size_t n, int src_type, int dst_type);
int pl_gather_f32(pl_ctx *ctx, const float *x, const int *idx, float *y, int outer, int axis_len, int inner, int n_idx);
int pl_erf_lut_f32(pl_ctx *ctx, float *x, const float *lut, float *y, size_t n);
int pl_instancenorm_f32(pl_ctx *ctx, float *x, const float *scale, const float *bias, int rows, int C, int inner,
                        double eps);
int pl_scatter_rows_f32(pl_ctx *ctx, float *dst, const long long *dst_row, const float *src, const int *src_row,
                        int n_rows, int row_len);
int pl_nonzero_count(pl_ctx *ctx, const void *x, size_t n, int elem_type, long long *scratch, long long *total);
int pl_nonzero_write(pl_ctx *ctx, const void *x, size_t n, int elem_type, const long long *scratch,
                     const long long *shape, int ndim, long long *out, long long total);
int pl_topk_f32(pl_ctx *ctx, const float *x, int outer, int n, int inner, int k, int largest, float *values,
                long long *indices);
int pl_lstm_cell_f32(pl_ctx *ctx, const float *gates_x, const float *gates_h, const float *bias, const float *c_prev,
                     float *h, float *c, int N, int H);
/* ---- a whole LSTM layer's recurrence ----
 * pl_lstm_seq_f32: the recurrent part of util.lstm (util.py:102-119) for L steps of ndir directions, after the input GEMMs.
 *   gates_x0, gates_x1  float32 (L N, 4H) per direction slot: row t N + n is x_t W^T of batch row n, gates in ONNX order
 *                     i | o | f | c.  gates_x1 is the second slot's and is null exactly when ndir == 1.
 *   R (ndir, 4H, H), bias (ndir, 8H) = Wb | Rb, h0 and c0 (ndir, N, H): the layer's operands as ONNX holds them.
 *   Y (L, ndir, N, H)   every step's h.  c (ndir, N, H): the cell state, updated in place; on return the final cell states.
 *                     c may be c0 itself; no other two operands may overlap.
 *   sign0             +1: slot 0 runs forward, -1: it runs in reverse.  Slot 1 always runs in reverse ("bidirectional" is
 *                     ndir = 2, sign0 = +1).
 *   time              launch s = 0 .. L-1 handles t = s in a forward slot and t = L-1-s in a reverse slot, both slots in the
 *                     same launch.  h_prev is Y[t-1][slot] (forward) or Y[t+1][slot] (reverse), and h0[slot] at s = 0; c_prev
 *                     is c[slot], and c0[slot] at s = 0.  The final h of a slot is Y[L-1][slot] (forward) or Y[0][slot].
 *   a step            gates = ((gates_x[t] + h_prev R^T) + bias[:4H]) + bias[4H:]; C = sigmoid(f) c_prev + sigmoid(i) tanh(c);
 *                     h = sigmoid(o) tanh(C); sigmoid(v) = 1 / (exp(-v) + 1); every product and sum rounded on its own: the
 *                     arithmetic of pl_lstm_cell_f32.  h_prev R^T is the 32 x 32 tile product of pl_gemm_f32's small-batch
 *                     form (trans_b, M <= 64, K >= 64, K % 8 == 0, aligned operands): K split over four waves in runs of
 *                     ceil((H / 8) / 4) 8-wide steps, 32x32x2 MFMAs, the partial tiles summed in the order 0, 1, 2, 3.  Where
 *                     pl_gemm_f32 takes that form the results are, bit for bit, those of pl_gemm_f32 + pl_lstm_cell_f32 per
 *                     step; everywhere they depend on the operands alone, never on a measured algorithm pick.
 * Asynchronous on ctx's stream: L launches of one kernel, grid (H / 8, ceil(N / 32), ndir), 256 threads; no host wait, no
 * allocation, no atomics, no synchronisation but the workgroup barrier and the kernel boundary: capturable into a hipGraph.
 * Rows at or past N are neither read nor written, and nothing but Y and c is written.
 * PL_EINVAL: a null pointer (other than gates_x1 at ndir == 1), gates_x1 given at ndir == 1, ndir outside {1, 2}, sign0 outside
 * {+1, -1}, L < 1, N < 0, H < 1, an operand that is not 16-byte aligned.  PL_EUNSUPPORTED: H % 8 != 0; N 4H >= 2^29 or
 * 4H H >= 2^29 (byte offsets of the buffer descriptors); N > 2097120 (65535 row blocks).  N == 0: PL_OK, no launch.  Every refusal comes before any launch and
 * leaves Y and c untouched. */
int pl_lstm_seq_f32(pl_ctx *ctx, const float *gates_x0, const float *gates_x1, const float *R, const float *bias,
                    const float *h0, const float *c0, float *Y, float *c, int L, int N, int H, int ndir, int sign0);
/* ---- tiled large-image inference: the device side of util.tile (util.py:291-348) ----
 * pl_resize_hwc_f32: util.resize (util.py:253-269) on an H x W x C image; ra/rs (OH entries) and
 * ca/cs (OW entries) are the integer sample rows/columns and their fractions, device arrays
 * computed by the host exactly as the reference does (float32 linspace, clip, floor).
 * pl_tile_accumulate_f32: one window's result (h x w x C) into the blend buffers at (r0, c0):
 * buf += rst * wt, count += wt with wt = min(distance to the window border, margin) + 1
 * (util.py:327-343).  pl_tile_normalise_f32: buf /= count (util.py:344). */
int pl_resize_hwc_f32(pl_ctx *ctx, const float *x, float *y, int H, int W, int C, int OH, int OW,
                      const int *ra, const float *rs, const int *ca, const float *cs);
int pl_tile_accumulate_f32(pl_ctx *ctx, const float *rst, float *buf, float *count, int h, int w,
                           int C, int r0, int c0, int OH, int OW, int margin);
int pl_tile_normalise_f32(pl_ctx *ctx, float *buf, const float *count, int OH, int OW, int C);
/* ---- uint8 image batches as net input ----
 * y[n][c][oh][ow] = fl(fl(r * k[c]) + b[c]), y the float32 (N, Co, OH, OW) tensor a net reads; call it in front of pl_plan_run.
 * x is a uint8 batch, (N, H, W, C) if nhwc else (N, C, H, W), and may start at any byte; C and Co in 1..4 (else
 * PL_EUNSUPPORTED).  Output channel c reads source channel order[c] (host array of Co ints, each in [0, C); NULL: identity, and
 * then Co == C).  k and b are host arrays of Co floats.  k, b and order travel as kernel arguments: nothing is allocated or
 * uploaded, the call is asynchronous on ctx's stream.
 * ra/rs (OH entries), ca/cs (OW entries): device tables as pl_resize_hwc_f32 takes them, all four or none.  None: OH == H,
 * OW == W and r is the byte as a float.  Given: r is util.resize's sample (util.py:253-269) of the bytes, columns first,
 * t = fl(fl(p[ca] * (1 - cs)) + fl(p[ca + 1] * cs)), then rows on t the same way; 1 - cs, 1 - rs in float32, no fused
 * multiply-add anywhere.  Tables need nhwc != 0 (else PL_EUNSUPPORTED) and H, W >= 2 (else PL_EINVAL: the reference's index
 * rule wraps there); entries are clamped to [0, H - 2] / [0, W - 2].
 * Limit: fewer than 2^31 source bytes and fewer than 2^31 output floats, else PL_EUNSUPPORTED.  Every refusal comes before any
 * launch and leaves y untouched.  Nothing outside x's N H W C bytes is read, nothing outside y's N Co OH OW floats written.
 * Without tables a workgroup takes PL_IMAGE_U8_TILE_PIXELS consecutive pixels of a plane (planes are flat: H W pixels), a lane
 * PL_IMAGE_U8_LANE_PIXELS of them, stored as one 16-byte word per channel plane where y is 16-byte aligned and H W % 4 == 0;
 * with tables a lane takes PL_IMAGE_U8_LANE_PIXELS consecutive columns of one output row (16-byte stores where OW % 4 == 0). */
#define PL_IMAGE_U8_TILE_PIXELS 1024
#define PL_IMAGE_U8_LANE_PIXELS 4
int pl_image_u8_nchw_f32(pl_ctx *ctx, const unsigned char *x, float *y, int N, int H, int W, int C, int nhwc,
                         int Co, const int *order, int OH, int OW, const int *ra, const float *rs, const int *ca,
                         const float *cs, const float *k, const float *b);
/* ---- uint8 images and label maps as net output ----
 * Both read x, the float32 (N, C, H, W) tensor a net wrote (any 4-byte boundary), and write uint8 y, which may start at any
 * byte; call them behind pl_plan_run, on the plan's context.  Asynchronous on ctx's stream; nothing is allocated or uploaded.
 *
 * pl_image_f32_u8: y is (N, H, W, Co) if nhwc else (N, Co, H, W), Co in 1..4 (else PL_EUNSUPPORTED), C >= 1.  Output channel c
 * reads source plane order[c] (host array of Co ints, each in [0, C); NULL: identity, and then Co == C).  k and b are host
 * arrays of Co floats and travel, with order, as kernel arguments.  Per sample, every operation rounded on its own:
 * t = fl(fl(v * k[c]) + b[c]); a NaN t becomes 0; t is clamped to [0, 255]; then rounded to nearest, ties to even (trunc == 0) or
 * truncated toward zero (trunc != 0); the byte is stored.  In numpy: np.where(np.isnan(t), 0, np.clip(t, 0, 255)), then
 * np.rint(..).astype(uint8) or .astype(uint8), bit for bit.
 *
 * pl_labels_f32_u8: y is (N, H, W).  2 <= C <= 256: y = np.argmax(x, axis=1) exactly (the first index among equal maxima, so
 * -0.0 and +0.0 tie; a NaN counts as the maximum, the first NaN wins; all -inf gives 0); threshold is ignored.  C == 1:
 * y = x > (float)threshold, a NaN gives 0.  C > 256: PL_EUNSUPPORTED.
 *
 * Limit: fewer than 2^31 source floats and fewer than 2^31 output bytes, else PL_EUNSUPPORTED.  N H W == 0: PL_OK, no launch.
 * Every refusal comes before any launch and leaves y untouched.  Nothing outside x's N C H W floats is read, nothing outside
 * y's bytes written; no atomics.
 * A workgroup takes PL_IMAGE_OUT_TILE_PIXELS consecutive pixels of one image's flat H W plane, a lane PL_IMAGE_OUT_LANE_PIXELS
 * of them: one 16-byte load per source plane where x is 16-byte aligned and H W % 4 == 0 (single floats otherwise); planar and
 * label bytes as one 32-bit store where their address is 4-byte aligned (single bytes otherwise); an interleaved tile as one run
 * of aligned 16-byte stores between single bytes in front of the first and behind the last 16-byte boundary. */
#define PL_IMAGE_OUT_TILE_PIXELS 1024
#define PL_IMAGE_OUT_LANE_PIXELS 4
int pl_image_f32_u8(pl_ctx *ctx, const float *x, unsigned char *y, int N, int C, int H, int W, int Co, const int *order,
                    int nhwc, const float *k, const float *b, int trunc);
int pl_labels_f32_u8(pl_ctx *ctx, const float *x, unsigned char *y, int N, int C, int H, int W, double threshold);
/* ---- tiled inference around a plan: windows cut and blended in one launch each ----
 * pl_tile_windows_*_nchw_f32: y, the float32 (S, Co, h, w) NCHW batch a plan reads, from ONE image x of (H, W, C), uint8 or
 * float32, at any byte / float boundary.  r0 / c0: device arrays of n >= 1 window origins in the working image of WH x WW pixels;
 * slot s shows window min(s, n - 1), so a short last chunk fills the plan's whole batch with defined data.  Window pixel (r, c)
 * is working pixel (r0 + r, c0 + c), clamped into the working image.  ra/rs (WH entries), ca/cs (WW entries): the tables of
 * pl_resize_hwc_f32 for (H, W) -> (WH, WW), all four or none.  None: WH == H, WW == W and the working image is x.  Given: a
 * working pixel is util.resize's sample of x with the roundings of pl_image_u8_nchw_f32 (columns first, every product and sum
 * rounded on its own), entries clamped to [0, H - 2] / [0, W - 2]; needs H, W >= 2.  The resampled image is never materialised.
 *   uint8:   y = fl(fl(r * k[c]) + b[c]) of source channel order[c]; C, Co in 1..4 (else PL_EUNSUPPORTED); order, k, b host arrays
 *            as pl_image_u8_nchw_f32 takes them (kernel arguments).
 *   float32: a copy of channel c; any C == Co >= 1.
 * A lane owns 4 consecutive pixels of one plane's flat h w pixels: one 16-byte store per channel where y is 16-byte aligned and
 * h w % 4 == 0, single floats otherwise.  Nothing outside x's H W C elements is read whatever the origins hold, nothing outside
 * y's S Co h w floats written.  Limit: fewer than 2^31 source elements and output floats, else PL_EUNSUPPORTED.  S == 0: PL_OK.
 *
 * pl_tile_blend_*: x holds all n = gr gc window results, float32 (n, C, oh, ow) as a plan wrote them, window i = gi gc + gj of
 * the row-major grid at output origin (R0[i], C0[i]) (device arrays).  Per output pixel and plane the covering windows are
 * visited in grid order: acc = fl(v w) for window 0, acc = fl(acc + fl(v w)) from +0.0 for the others, count = the integer sum
 * of w, result fl(acc / (float)count), w = min(distance to the window's nearest edge, ramp) + 1: the reference's float32 loop
 * (util.py:327-344: window 0 assigned, the others added to zeros) bit for bit, a -0.0 under window 0 alone included.  Any number of windows may cover a pixel; a pixel none covers gets 0 / 0.
 * count must stay below 2^24 (the host keeps it within the reference's uint16).  One launch, no atomics, no zero-fill, no
 * weight plane; every output element is written once.
 *   pl_tile_blend_f32:       y float32 (OH, OW, C).
 *   pl_tile_blend_u8:        y uint8 (OH, OW, Co) if nhwc else (Co, OH, OW), the blended value of plane order[c] through
 *                            pl_image_f32_u8's rule (Co, order, k, b, trunc as there).
 *   pl_tile_blend_labels_u8: y uint8 (OH, OW), pl_labels_f32_u8's rule on the blended values (C > 256: PL_EUNSUPPORTED).
 * Limit: fewer than 2^31 window floats and output elements.  Every refusal comes before any launch. */
int pl_tile_windows_u8_nchw_f32(pl_ctx *ctx, const unsigned char *x, float *y, int H, int W, int C, int Co, const int *order,
                                const int *r0, const int *c0, int n, int S, int h, int w, int WH, int WW, const int *ra,
                                const float *rs, const int *ca, const float *cs, const float *k, const float *b);
int pl_tile_windows_f32_nchw_f32(pl_ctx *ctx, const float *x, float *y, int H, int W, int C, const int *r0, const int *c0, int n,
                                 int S, int h, int w, int WH, int WW, const int *ra, const float *rs, const int *ca,
                                 const float *cs);
int pl_tile_blend_f32(pl_ctx *ctx, const float *x, float *y, int n, int C, int oh, int ow, const int *R0, const int *C0, int gr,
                      int gc, int OH, int OW, int ramp);
int pl_tile_blend_u8(pl_ctx *ctx, const float *x, unsigned char *y, int n, int C, int oh, int ow, const int *R0, const int *C0,
                     int gr, int gc, int OH, int OW, int ramp, int Co, const int *order, int nhwc, const float *k,
                     const float *b, int trunc);
int pl_tile_blend_labels_u8(pl_ctx *ctx, const float *x, unsigned char *y, int n, int C, int oh, int ow, const int *R0,
                            const int *C0, int gr, int gc, int OH, int OW, int ramp, double threshold);
/* ---- detections as net output ----
 * YOLO-style heads -> rows [x1, y1, x2, y2, score, class]: pl_yolo_decode_f32 once per head, pl_topk_f32 over the scores,
 * pl_nms_f32.  Call them behind pl_plan_run, on the plan's context.  Asynchronous on ctx's stream; nothing is allocated or
 * uploaded, nothing synchronises, no atomics.
 *
 * pl_yolo_decode_f32: x is one head, float32 (N, A (5 + C), Gh, Gw); anchors is a host array of 2 A floats (aw, ah per anchor, in
 * input pixels) and travels as kernel arguments, A <= PL_YOLO_MAX_ANCHORS.  An image's anchors of all heads form a row of `row`
 * entries; this head's start at `offset`, anchor a of cell (gy, gx) has index i = offset + (a Gh + gy) Gw + gx and is stored
 * at position row - 1 - i of the image's row, back to front: pl_topk_f32 (largest = 1) orders equal values by descending
 * position, so its result is by (score descending, anchor index ascending).  With
 * t[j] = x[n, a (5 + C) + j, gy, gx] and s(v) = 1 / (1 + exp(-v)) (pl_sigmoid_f32's):
 *   class = argmax of t[5 : 5 + C] with pl_labels_f32_u8's rule (the first of equal maxima, the first NaN before any number),
 *   score = fl(s(t4) * s(t[5 + class])); the anchor is a candidate iff score > (float)conf (a NaN score is none),
 *   cx = fl(fl(s(t0) + gx) * (float)sx), cy likewise with gy and sy, w = fl(exp(t2) * aw), h = fl(exp(t3) * ah),
 *   box = (cx - w/2, cy - h/2, cx + w/2, cy + h/2), not clipped; every operation rounded on its own.
 * A candidate writes scores (N, row), classes (N, row) int32 and boxes (N, row, 4); any other anchor writes score -1 and leaves
 * its class and box untouched.  One lane per cell of one anchor; the class planes are read only where s(t4) > conf.
 *
 * pl_nms_f32: greedy non-maximum suppression of each image's K entries (sorted_scores (N, K) descending and order (N, K) int64,
 * rows of boxes (N, R, 4) / classes (N, R) int32, as pl_topk_f32 returns them; classes NULL: one class).  Entry j is a candidate
 * iff its score > (float)floor and 0 <= order < R.  In order, a candidate is dropped when a candidate kept earlier (class_aware:
 * of the same class) overlaps it: in float32, every operation rounded on its own, fmin / fmax as np.fmin / np.fmax,
 *   iw = fmax(0, fmin(x2i, x2j) - fmax(x1i, x1j)), ih likewise, inter = iw ih, area = (x2 - x1) (y2 - y1),
 *   union = (area_i + area_j) - inter, dropped iff inter > (float)iou * union
 * (no division: a zero union or a NaN drops nothing); it stops after max_det kept.  det (N, max_det, 6) gets the kept rows
 * [x1, y1, x2, y2, score, class] and +0.0 in the rows behind them, num (N) int32 their count: both are written completely.
 * One workgroup per image, 24 K + 16 ceil(K / 64) bytes of dynamic LDS, one barrier per kept box.
 *
 * PL_EINVAL: a null pointer (classes of pl_nms_f32 excepted), a negative dimension, C < 1, offset < 0 or offset + A Gh Gw > row,
 * K > R.  PL_EUNSUPPORTED: A > PL_YOLO_MAX_ANCHORS, K > PL_NMS_MAX_CANDIDATES, max_det > K, 2^31 or more floats in a tensor.
 * N == 0 (decode: or A Gh Gw == 0): PL_OK, no launch.  Every refusal comes before any launch and leaves the outputs untouched. */
#define PL_YOLO_MAX_ANCHORS 8
#define PL_NMS_MAX_CANDIDATES 4096
int pl_yolo_decode_f32(pl_ctx *ctx, const float *x, int N, int A, int C, int Gh, int Gw, const float *anchors, double sx,
                       double sy, double conf, int row, int offset, float *scores, int *classes, float *boxes);
int pl_nms_f32(pl_ctx *ctx, const float *boxes, const int *classes, const float *sorted_scores, const long long *order, int N,
               int R, int K, double floor, double iou, int class_aware, int max_det, float *det, int *num);
/* ---- objects as net output ----
 * pl_components_u8_i32: connected components of the uint8 class map m (N, H, W) -- pl_labels_f32_u8's output, or any label map --
 * and the region table of each image's first max_objects objects.  An object is a maximal set of pixels of one image with equal
 * class other than `background` (0..255, or -1: every pixel belongs to an object), joined through 4- or 8-neighbour steps
 * (`connectivity`); pixels of different images, and the last pixel of a row and the first of the next, are no neighbours.
 *   labels    int32 (N, H, W): 0 on background, else the object's number 1, 2, ... per image, objects numbered by the raster
 *             position y W + x of their first pixel (scipy.ndimage.label's numbering for a binary map; the same rule over all
 *             classes together otherwise).
 *   num       int32 (N): the objects of each image; it may exceed max_objects.
 *   objects   int32 (N, max_objects, 6): row j is object j + 1, [class, area, y0, x0, y1, x1], the box half-open; rows at and
 *             behind num are 0.  Objects numbered above max_objects keep their number in labels and have no row.
 *   centroids float32 (N, max_objects, 2): [cy, cx] = float32(float64(sum of y) / float64(area)), the sums exact integers, one
 *             IEEE double division, one rounding; +0.0 in the unused rows.
 * Everything is exact and unique: nothing depends on the order in which atomics land.  All four outputs are written completely
 * and nothing relies on zeroed memory.  Asynchronous on ctx's stream; seven launches (six where max_objects == 0, one fewer
 * where the image is a single tile), no host wait, no host-computed value: capturable into a hipGraph.
 * scratch: PL_CC_SCRATCH_BYTES(N, H, W, max_objects) bytes of the caller's, 8-byte aligned, contents irrelevant.
 * A workgroup of the tile passes takes PL_CC_TILE_H x PL_CC_TILE_W pixels; roots are counted per PL_CC_BLOCK raster-consecutive
 * pixels and one workgroup per image scans those counts PL_CC_SCAN_STEP at a time.
 * PL_EINVAL: a null pointer (objects / centroids may be NULL when max_objects == 0), a negative dimension or max_objects,
 * connectivity other than 4 or 8, background outside -1..255.  PL_EUNSUPPORTED: H W >= 2^31 or N H W >= 2^31,
 * max_objects > PL_CC_MAX_OBJECTS, N max_objects 6 >= 2^31.  N == 0 or H W == 0: PL_OK, no launch.  Every refusal comes before any
 * launch and leaves the outputs untouched. */
#define PL_CC_TILE_H 32
#define PL_CC_TILE_W 64
#define PL_CC_BLOCK 2048
#define PL_CC_SCAN_STEP 1024
#define PL_CC_MAX_OBJECTS 65536
#define PL_CC_SCRATCH_BYTES(N, H, W, max_objects)                                                        \
    ((size_t)(N) * (size_t)(max_objects) * 16 + (size_t)(N) * (size_t)(H) * (size_t)(W) * 4 +            \
     (size_t)(N) * (((size_t)(H) * (size_t)(W) + PL_CC_BLOCK - 1) / PL_CC_BLOCK) * 4)
int pl_components_u8_i32(pl_ctx *ctx, const unsigned char *m, int N, int H, int W, int connectivity, int background,
                         int max_objects, void *scratch, int *labels, int *num, int *objects, float *centroids);
/* ---- keypoints as net output ----
 * pl_peaks_f32: the local maxima of every plane of the float32 heat maps x (N, K, H, W), counted, and the best max_peaks of each
 * plane as points.  Pixel p = y W + x of a plane is a peak iff v[p] > threshold holds and, for each of its up to eight
 * neighbours q inside the same plane (planes and images are no neighbours, nor are a row's last pixel and the next row's first),
 *   ties == PL_PEAKS_TIES_ALL:   v[p] >= v[q]  (maxpool 3x3 with -inf padding == the map),
 *   ties == PL_PEAKS_TIES_FIRST: v[p] > v[q] where q < p, v[p] >= v[q] where q > p  (of a plateau, the pixel that comes first).
 * The comparisons are IEEE float32: a NaN pixel is no peak, a NaN neighbour cancels one, -0.0 ties with +0.0.  A plane's peaks
 * are ordered by score descending, equal scores (IEEE ==) by ascending p.
 *   num   int32 (N, K): all peaks of the plane; it may exceed max_peaks.
 *   peaks float32 (N, K, max_peaks, 3): row j < min(num, max_peaks) is the j-th peak, [x, y, score]; the rows behind are +0.0.
 *         score carries the pixel's own bits.  x = fl(fl(px + dx) * fl(sx)), y = fl(fl(py + dy) * fl(sy)); px + dx is exact, so
 *         the product is the single rounding.  refine == PL_PEAKS_REFINE_NONE: dx = dy = 0.  PL_PEAKS_REFINE_QUARTER:
 *         dx = +0.25 if v[py, px + 1] > v[py, px - 1] holds, -0.25 if < holds, else 0, and 0 at px == 0 or px == W - 1; dy
 *         likewise along y.
 * Everything is exact and unique.  Both outputs are written completely and nothing relies on zeroed memory.  Asynchronous on
 * ctx's stream; two launches (one where H W == 0), no global atomics, no host wait: capturable into a hipGraph.
 * scratch: PL_PEAKS_SCRATCH_BYTES(N, K, H, W, max_peaks) bytes of the caller's, 8-byte aligned, contents irrelevant.
 * A workgroup of the first launch takes a PL_PEAKS_TILE_H x PL_PEAKS_TILE_W tile of one plane and hands on its best max_peaks; one
 * workgroup per plane then merges the tiles' candidates, PL_PEAKS_MERGE_KEYS of them in one sort, more in rounds.
 * PL_EINVAL: a null pointer, a negative dimension, max_peaks < 1, ties or refine outside their codes, a NaN threshold or stride.
 * PL_EUNSUPPORTED: max_peaks > PL_PEAKS_MAX_PEAKS, H or W above PL_PEAKS_MAX_EXTENT (below it px + 0.25 is exact in float32),
 * H W >= 2^31, N K H W >= 2^31, 3 N K max_peaks >= 2^31.  N K == 0: PL_OK, no launch; H W == 0: num = 0 and +0.0 rows.  Every
 * refusal comes before any launch and leaves the outputs untouched. */
#define PL_PEAKS_TILE_H 32
#define PL_PEAKS_TILE_W 64
#define PL_PEAKS_MAX_PEAKS 256
#define PL_PEAKS_MERGE_KEYS 2048
#define PL_PEAKS_MAX_EXTENT 4194304
#define PL_PEAKS_TIES_ALL 0
#define PL_PEAKS_TIES_FIRST 1
#define PL_PEAKS_REFINE_NONE 0
#define PL_PEAKS_REFINE_QUARTER 1
#define PL_PEAKS_SCRATCH_BYTES(N, K, H, W, max_peaks)                                                                  \
    ((size_t)(N) * (size_t)(K) * (((size_t)(H) + PL_PEAKS_TILE_H - 1) / PL_PEAKS_TILE_H) *                             \
     (((size_t)(W) + PL_PEAKS_TILE_W - 1) / PL_PEAKS_TILE_W) * ((size_t)(max_peaks) * 8 + 4))
int pl_peaks_f32(pl_ctx *ctx, const float *x, int N, int K, int H, int W, double threshold, int ties, int max_peaks, int refine,
                 double sy, double sx, void *scratch, float *peaks, int *num);
/* ---- instances as net output ----
 * pl_flow_instances_f32: instance masks by flow following.  Per image three float32 planes over (H, W): a flow field dy, dx and
 * a probability prob; element (n, plane, y, x) is x[n image_stride + off_plane + (y W + x) pixel_stride]  (NCHW: pixel_stride 1,
 * off = c H W; an (H, W, C) map: pixel_stride C, off = c).  Pixel p = y W + x.  fl() is one float32 rounding, nothing is
 * contracted into an FMA.
 *   1. fg[p] iff prob[p] > (float)level  (a NaN is background).
 *   2. ay = fl(dy dy), ax = fl(dx dx), l2 = fl(ay + ax).  p moves iff fg[p] and l2 > g2 = fl((float)min_flow (float)min_flow)  (a NaN
 *      l2 does not move).  sy = sign(dy) if fl(3 ay) >= ax else 0, sx = sign(dx) if fl(3 ax) >= ay else 0: the unit vector's
 *      components rounded half away from zero, eight directions, total on inf.  t = (clamp(y + sy, 0, H - 1), clamp(x + sx, 0, W - 1)).
 *      next[p] = t if p moves and fg[t], else p: trajectories never leave the foreground.
 *   3. end[p] = next applied exactly 2^rounds times (`rounds` pointer doublings, each from one buffer into another): fixed points
 *      stay, pixels on a cycle land where 2^rounds steps take them.
 *   4. cnt[q] = the foreground p with end[p] == q; the sink map cnt > 0 is labelled by pl_components_u8_i32 (connectivity 8): S, nS.
 *   5. The raw instance of a foreground p is S[end[p]], vol[j] its pixel count  (at most PL_FLOW_MAX_RAW(H, W) raw instances).
 *   6. Instance j is kept iff vol[j] >= min_size; the kept ones are renumbered 1, 2, ... in ascending j.
 *   masks     int32 (N, H, W): the new number; 0 on background and on dropped instances.
 *   num       int32 (N): the kept instances of each image; it may exceed max_instances.
 *   instances int32 (N, max_instances, 5): row j is instance j + 1, [area, y0, x0, y1, x1], the box half-open; rows at and behind
 *             num are 0.  Instances numbered above max_instances keep their number in masks and have no row.
 *   centres   float32 (N, max_instances, 2): [cy, cx] = float32(float64(sum of y) / float64(area)); +0.0 in the unused rows.
 * Everything is exact and unique: nothing depends on the order in which atomics land.  All four outputs are written completely
 * and nothing relies on zeroed memory.  Asynchronous on ctx's stream; step, ceil(rounds / 2) doublings (two fused per launch),
 * count, sink map, the components chain, volume, renumber, table and centres (none where max_instances == 0); no host wait, no
 * host-computed value: capturable into a hipGraph.
 * scratch: PL_FLOW_SCRATCH_BYTES(N, H, W, max_instances) bytes of the caller's, 8-byte aligned, contents irrelevant: coordinate
 * sums, two pointer buffers, hit counts, sink labels, the volume table, the sink map and the components chain's scratch.
 * The table pass takes the components tile, PL_CC_TILE_H x PL_CC_TILE_W pixels per workgroup; one workgroup per image renumbers
 * PL_FLOW_SCAN_STEP raw instances at a time.
 * PL_EINVAL: a null pointer (instances / centres may be NULL when max_instances == 0), a negative dimension, rounds, min_size or
 * max_instances, a stride <= 0, a negative offset, a NaN level or min_flow.  PL_EUNSUPPORTED: H W >= 2^31 or N H W >= 2^31,
 * rounds > PL_FLOW_MAX_ROUNDS, max_instances > PL_FLOW_MAX_INSTANCES, N max_instances 5 >= 2^31.  N == 0 or H W == 0: PL_OK, no
 * launch.  Every refusal comes before any launch and leaves the outputs untouched. */
#define PL_FLOW_SCAN_STEP 1024
#define PL_FLOW_MAX_ROUNDS 30
#define PL_FLOW_MAX_INSTANCES 65536
#define PL_FLOW_ALIGN(bytes) (((size_t)(bytes) + 15) / 16 * 16)
#define PL_FLOW_MAX_RAW(H, W) ((((size_t)(H) + 1) / 2) * (((size_t)(W) + 1) / 2))
#define PL_FLOW_SCRATCH_BYTES(N, H, W, max_instances)                                                                  \
    (16 + (size_t)(N) * (size_t)(max_instances) * 16 + 4 * PL_FLOW_ALIGN((size_t)(N) * (size_t)(H) * (size_t)(W) * 4) + \
     PL_FLOW_ALIGN((size_t)(N) * PL_FLOW_MAX_RAW(H, W) * 4) + PL_FLOW_ALIGN((size_t)(N) * 4) +                         \
     PL_FLOW_ALIGN((size_t)(N) * (size_t)(H) * (size_t)(W)) + PL_CC_SCRATCH_BYTES(N, H, W, 0))
int pl_flow_instances_f32(pl_ctx *ctx, const float *x, int N, int H, int W, long long image_stride, long long pixel_stride,
                          long long off_dy, long long off_dx, long long off_prob, double level, double min_flow, int rounds,
                          int min_size, int max_instances, void *scratch, int *masks, int *num, int *instances, float *centres);
/* ---- text as net output ----
 * pl_ctc_greedy_f32: greedy CTC decoding of S = S_outer S_inner sequences of T frames over C classes.  Element (so, si, t, c) of
 * the float32 x is at so st_outer + si st_inner + t st_time + c st_class, strides in elements; sequence s = so S_inner + si.  The
 * layouts are stride sets: (T, N, C) is S_outer = N, S_inner = 1, st_outer = C, st_time = N C, st_class = 1; (N, T, C) is
 * st_outer = T C, st_time = C; (N, C, H, W) with a line per (n, h) and time along W is S_outer = N, S_inner = H,
 * st_outer = C H W, st_inner = W, st_time = 1, st_class = H W.
 *   frame label       numpy's argmax over the C classes of frame (s, t): the first of equal maxima, the first NaN before any
 *                     number, -0.0 ties with +0.0 (the rule of pl_labels_f32_u8).
 *   frame confidence  with m the frame's maximum.  PL_TEXT_CONF_SOFTMAX: 1 / sum_c exp(x_c - m), NaN when m is not finite (the
 *                     one result that is not exact: a float32 sum in the kernel's order).  PL_TEXT_CONF_VALUE: the bits of x at
 *                     the argmax.  PL_TEXT_CONF_NONE: +0.0, and the exponentials are skipped.
 *   valid length      len[s] = min(lengths[s], T), a negative lengths[s] counting as 0; T where lengths is null.  Frames at or
 *                     past len do not exist: they are neither read nor decoded.
 *   symbols           frame t < len starts a symbol iff label[t] != blank and (t == 0 or label[t] != label[t - 1] or
 *                     merge_repeated == 0).  Its run ends at the first later frame whose label differs, or at len; with
 *                     merge_repeated == 0 at t + 1.
 *   length int32 (S): all symbols of the sequence; it may exceed max_len.
 *   text   int32 (S, max_len): the labels of the first max_len symbols, -1 behind them.
 *   conf   float32 (S, max_len): the confidence of each symbol's first frame, +0.0 behind.
 *   spans  int32 (S, max_len, 2): [start, end) in frames, 0 behind.
 * All four are written completely and nothing relies on zeroed memory.  Asynchronous on ctx's stream; two launches, a frame pass
 * and a collapse pass (one where S T == 0), no global atomics, no host wait: capturable into a hipGraph.
 * scratch: PL_TEXT_SCRATCH_BYTES(S, T) bytes of the caller's, 4-byte aligned, contents irrelevant: frame labels, then frame
 * confidences.
 * The frame pass has two forms.  st_class == 1: a frame is a row of C floats, read once in 16-byte words between a peeled head
 * and tail, by one wave where C <= PL_TEXT_ROW_WAVE_MAX and by a workgroup above.  Otherwise a workgroup takes
 * PL_TEXT_TIME_LANES consecutive frames of a sequence and splits the classes over its PL_TEXT_TIME_GROUPS lane groups.
 * The collapse pass is one workgroup per sequence, PL_TEXT_CHUNK frames at a time.
 * PL_EINVAL: a null pointer other than lengths, a negative dimension, C < 1, blank outside [0, C), max_len < 1, a confidence
 * code outside PL_TEXT_CONF_*.  PL_EUNSUPPORTED: max_len > PL_TEXT_MAX_LEN, T > PL_TEXT_MAX_FRAMES (2^20: a collapse
 * workgroup walks at most 4096 chunks), S T C >= 2^31.  S == 0: PL_OK, no launch; T == 0: length = 0 and the filler rows.  Every
 * refusal comes before any launch and leaves the outputs untouched. */
#define PL_TEXT_MAX_LEN 1024
#define PL_TEXT_MAX_FRAMES 1048576
#define PL_TEXT_CHUNK 256
#define PL_TEXT_ROW_WAVE_MAX 1024
#define PL_TEXT_TIME_LANES 32
#define PL_TEXT_TIME_GROUPS 32
#define PL_TEXT_CONF_NONE 0
#define PL_TEXT_CONF_SOFTMAX 1
#define PL_TEXT_CONF_VALUE 2
#define PL_TEXT_SCRATCH_BYTES(S, T) ((size_t)(S) * (size_t)(T) * 8)
int pl_ctc_greedy_f32(pl_ctx *ctx, const float *x, int S_outer, int S_inner, int T, int C, long long st_outer, long long st_inner,
                      long long st_time, long long st_class, const int *lengths, int blank, int merge_repeated, int confidence,
                      int max_len, void *scratch, int *text, int *length, float *conf, int *spans);
/* split-K combine + epilogue (internal to conv, exported for tests) */
int pl_splitk_reduce_f32(pl_ctx *ctx, const float *ws, int splits, float *y,
                         int N, int C, int inner, const float *bias,
                         const float *scale, const float *shift,
                         const float *res, int act, double alpha);
/* The streaming kernels launch at most 8 blocks of 256 threads per CU and stride over the rest; those that count in 32 bits
 * accept `total` work items only if no counter can wrap: total + blocks * 256 <= 2^32.  *ok = that verdict for a device of
 * cu_count CUs (<= 0: 256).  Host query, no device. */
int pl_stream_loop32_ok(size_t total, int cu_count, int *ok);

/* ---- multi-GPU (RCCL over xGMI): one process per GPU -------------------- */
/* The reference has no distributed code.  The forward pass shards by batch
 * with no collectives; the ONE exchange is the weight blob broadcast at load
 * time (net.load_weights, net.py:83-88). */
#define PL_UNIQUE_ID_BYTES 128
int pl_comm_unique_id(void *id_out);                /* rank 0 */
int pl_comm_init_rank(pl_ctx *ctx, int world, int rank, const void *id);
int pl_comm_bcast(pl_ctx *ctx, void *buf, size_t bytes, int root);
int pl_comm_allreduce_max_f32(pl_ctx *ctx, float *buf, size_t n); /* in place, device */
int pl_comm_allgather(pl_ctx *ctx, const void *send, void *recv, size_t bytes_per_rank);
/* what RCCL itself says about the communicator: ncclCommCount / ncclCommUserRank (run reports: config.rccl_ranks) */
int pl_comm_info(pl_ctx *ctx, int *ranks, int *rank);
int pl_comm_destroy(pl_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* PLANER_HIP_H */
