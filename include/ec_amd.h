/*
 * ec_amd.h -- C-ABI of the MI355X-native embodied-clip hot path.
 *
 * The reference (allenai/embodied-clip) is pure Python over torch.nn and has
 * NO FFI / operator-registration boundary of its own.  This
 * header is therefore the boundary a maintainer would bind (ctypes stubs are
 * shown in INTEGRATION.md); every entry point cites the reference-side
 * interface it replaces.  "[U]" = upstream module that the reference depends
 * on but does not vendor (openai/CLIP @40f5484c, allenai/allenact ~v0.5.0).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no torch / HIP types in signatures
 *     (ec_stream_t is a hipStream_t passed as void*; NULL = default stream).
 *   - every pointer is a DEVICE pointer unless the name starts with h_.
 *   - functions return EC_OK (0) or a negative EC_ERR_* code; they never throw
 *     and never allocate behind the caller's back: workspaces are sized by an
 *     ec_*_workspace_bytes() query and passed in.
 *   - kernels are enqueued on the given stream and are asynchronous.
 *   - one handle per process/GPU; handles are immutable after creation and may
 *     be used from one thread at a time.
 *   - "bf16" buffers are raw uint16 bfloat16; activations are NHWC
 *     (channels-last), conv weights are [Cout][KH][KW][Cin].
 */
#ifndef EC_AMD_H
#define EC_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* ec_stream_t;
typedef void* ec_event_t;    /* hipEvent_t */

enum {
    EC_OK = 0,
    EC_ERR_ARG = -1,         /* null pointer / bad enum */
    EC_ERR_SHAPE = -2,       /* unsupported shape for this kernel */
    EC_ERR_LAUNCH = -3,      /* HIP launch failed */
    EC_ERR_WORKSPACE = -4,   /* workspace too small */
    EC_ERR_ALLOC = -5,       /* host allocation failed */
    EC_ERR_UNSUPPORTED = -6
};

enum { EC_ACT_NONE = 0, EC_ACT_RELU = 1, EC_ACT_QUICKGELU = 2 };

int ec_version(void);
const char* ec_strerror(int code);

/* Stream plumbing for callers that keep several launches in flight (no reference counterpart: the reference runs on one
 * stream).  The HIP runtime binds a stream to one of its few hardware queues at the stream's FIRST submission; two streams on
 * the same queue run one after the other.  ec_bind_streams gives each of `n` freshly created streams its first work (a
 * spin kernel of `spin_us`) while the others are busy, so that each gets a queue of its own; ec_stream_pair_overlap
 * measures a pair: *ratio ~ 1 = concurrent, ~ 2 = serialised.  Both block (device synchronise): set-up time only. */
int ec_bind_streams(ec_stream_t* streams, int n, int spin_us);
int ec_stream_pair_overlap(ec_stream_t a, ec_stream_t b, int spin_us, float* ratio);

/* ------------------------------------------------------------------------
 * Encoder building blocks (bf16 storage, fp32 accumulate on MFMA).
 * Replace the cuDNN/cuBLAS kernels the reference triggers through
 * `clip_model(clip_input)` (primitive_probing/generate_data/thor_image_features.py:109).
 * ---------------------------------------------------------------------- */

/* Conv (1x1 or 3x3, stride 1, pad (k-1)/2) with BatchNorm folded into
 * (w,bias) per freeze_model (thor_image_features.py:26-33), fused
 * + bias, + residual, activation, and optional fused AvgPool2d(2) epilogue
 * ([U] clip/model.py Bottleneck.forward: conv-bn-relu / avgpool / add-relu).
 * in  bf16 [B,H,W,Cin]; w bf16 [Cout][k*k*Cin]; bias f32 [Cout];
 * res bf16 [B,H,W,Cout] or NULL (not with pool); out bf16 [B,H',W',Cout]
 * (H'=H/2 when pool).  Cin power of two >= 8; Cout multiple of 32. */
int ec_conv_bf16(const void* in, const void* w, const float* bias, const void* res, void* out,
                 int B, int H, int W, int Cin, int Cout, int ksize, int pool, int act,
                 ec_stream_t stream);
/* ec_conv_bf16 writing a COLUMN BLOCK of a wider tensor: output row m starts at out + m * out_row_stride (elements;
 * >= Cout, multiple of 8; == Cout is ec_conv_bf16).  The trunk lays a stride-2 Bottleneck's pooled conv2 output
 * [M, planes] and its pooled block input [M, inplanes] (ec_avgpool2_bf16_ld) side by side, so that conv3 and the
 * downsample conv of [U] clip/model.py Bottleneck.forward (`out = relu(bn3(conv3(out)) + downsample(x))`) are ONE GEMM
 * over the concatenated K axis: the downsample output is never written or re-read. */
int ec_conv_bf16_ld(const void* in, const void* w, const float* bias, const void* res, void* out,
                    int B, int H, int W, int Cin, int Cout, int ksize, int pool, int act, int out_row_stride,
                    ec_stream_t stream);
/* Plain GEMM view of the same kernel: out[M,N] = act(A[M,K] W[N,K]^T + bias (+res)).
 * Replaces nn.Linear / nn.MultiheadAttention projections of [U] clip/model.py
 * ResidualAttentionBlock and AttentionPool2d.  K multiple of 8, N multiple of 32. */
int ec_gemm_bf16(const void* A, const void* W, const float* bias, const void* res, void* out,
                 int M, int N, int K, int act, ec_stream_t stream);

/* ------------------------------------------------------------------------
 * Transformer tower stages, one at a time (vit.hip).  ec_vit_forward / ec_text_forward issue every stage through the
 * same launch code; these entries exist so that each kernel can be tested alone against a float64 reference
 * (tests/test_gpu_vit_stages.py), as ec_gemm_f32 / ec_split3_bf16 / ec_dw_tn_x3 expose the policy's inner GEMMs.
 * Arguments are checked before any HIP call: NULL -> EC_ERR_ARG, a refused geometry -> EC_ERR_SHAPE.
 *   ec_mha_bf16: softmax(q k^T / 8 [+ causal mask]) v per (sequence, head) of [U] clip/model.py
 *     ResidualAttentionBlock.attention; qkv bf16 [B*L, 3D] (q | k | v, head h at columns 64 h..), out bf16 [B*L, D].
 *     Non-causal L <= 64 runs the MFMA core, everything else the general LDS core.  D / heads == 64, 1 <= L <= 512.
 *   ec_layernorm_bf16: nn.LayerNorm(D), eps 1e-5, bf16 rows in and out, fp32 gamma / beta.  D % 64 == 0, D <= 1024.
 *   ec_vit_assemble_bf16: row t of frame b = ln_pre((t == 0 ? cls : pemb[b, t - 1]) + pos[t]); pemb bf16 [B*(L-1), D],
 *     cls f32 [D], pos f32 [L, D].  stats_or_null: f32 [B*L][4], the record {sum, M2, D, 0} of every ROUNDED output
 *     row.  Same widths, L >= 2.
 *   ec_row_stats_bf16: the record {sum, M2, D, 0} of every bf16 row of x [rows, D].  Same widths.
 *   ec_ln_fold_bf16: a LayerNorm folded into the Linear that consumes it: W bf16 [N, K], b f32 [N] ->
 *     Wg = bf16(W diag(gamma)) [N, K], s[n] = sum_k Wg[n, k], c[n] = sum_k beta[k] W[n, k] + b[n].
 *   ec_gemm_bf16_ln: the 8-wave GEMM with LayerNorm folded in.  Consumer (ln_s != NULL, no res): out = act(rstd (A Wt^T -
 *     mean ln_s) + bias) with Wt / ln_s / bias = Wg / s / c of ec_ln_fold_bf16 and the rows' mean / rstd (eps 1e-5)
 *     combined from the ln_np (1..8) records per row in ln_stats [M][ln_np][4].  Producer (stats_out != NULL):
 *     out = act(A Wt^T + bias (+ res)) and one record per row and column tile into stats_out [M][*np_out][4]
 *     (*np_out = N / 128 or N / 256, at most 8).  N % 128 == 0, K % 64 == 0.
 * ---------------------------------------------------------------------- */
int ec_mha_bf16(const void* qkv, void* out, int B, int L, int D, int heads, int causal, ec_stream_t stream);
int ec_layernorm_bf16(const void* x, const float* gamma, const float* beta, void* out, long rows, int D, ec_stream_t stream);
int ec_vit_assemble_bf16(const void* pemb, const float* cls, const float* pos, const float* gamma, const float* beta, void* out,
                         float* stats_or_null, int B, int L, int D, ec_stream_t stream);
int ec_row_stats_bf16(const void* x, float* stats, long rows, int D, ec_stream_t stream);
int ec_ln_fold_bf16(const void* W, const float* gamma, const float* beta, const float* b, void* Wg, float* s, float* c, int N,
                    int K, ec_stream_t stream);
int ec_gemm_bf16_ln(const void* A, const void* Wt, const float* bias, const void* res, void* out, int M, int N, int K, int act,
                    const float* ln_s, const float* ln_stats, int ln_np, float* stats_out, int* np_out, ec_stream_t stream);

/* ------------------------------------------------------------------------
 * CLIP image preprocessing on raw uint8 frames: Resize(n_px, BICUBIC) + CenterCrop(n_px), bit-exact with Pillow.
 * Replaces the PIL/torchvision half of `clip_preprocess(frame)` (primitive_probing/generate_data/
 * thor_image_features.py:108, :36-44; frames are 300x300: thor_frames.py:33-34).  ToTensor + Normalize are fused into
 * the stem (ec_rn50_forward_u8).
 *   ec_clip_resize_table_ints / ec_clip_resize_table: HOST ONLY -- torchvision's resize / center-crop geometry and
 *     Pillow's two 22-bit fixed-point coefficient tables (libImaging/Resample.c precompute_coeffs +
 *     normalize_coeffs_8bpc) for H x W frames; table[6] = the LDS rows the kernel needs (pass as table_max_rows).
 *     The caller copies the table to the device once per frame geometry.
 *   ec_clip_resize_crop_u8: frames uint8 [B, H, W, 3] -> uint8 [B, n_px, n_px, 3].
 * ---------------------------------------------------------------------- */
size_t ec_clip_resize_table_ints(int H, int W, int n_px);
int ec_clip_resize_table(int H, int W, int n_px, int* host_table, size_t n_ints);
int ec_clip_resize_crop_u8(const uint8_t* frames_u8, const int* table_dev, int table_max_rows, uint8_t* out_u8, int B,
                           int H, int W, int n_px, ec_stream_t stream);

/* ------------------------------------------------------------------------
 * Probe labels from the simulator's semantic-segmentation frame (labels.hip).  Replaces the numpy labelling of
 * primitive_probing/generate_data/thor_image_features.py:71-88,115-127: `class_mask` (all three channels equal the
 * class colour; a class without a colour has an empty mask, :72-73), `obj_presence` over the whole frame (:122) and
 * over the nine `grid_bboxes` cells (:80-88,123-127; cell (i, j) = rows [floor(i*H/3), floor((i+1)*H/3)), columns
 * likewise).
 *   sem_u8       uint8 [B, H, W, 3]   point['semantic_frame']
 *   colors_u8    uint8 [B, C, 4]      r, g, b, valid per target class of THAT frame (object_id_to_color is stored per
 *                                     point, :118); valid == 0: the class has no colour.  Classes may share a colour.
 *   presence     int64 [B, C]         0 / 1
 *   localization int64 [B, 9, C]      0 / 1, cells row-major over (y, x)
 * Integer equality throughout: exact, and independent of how frames are batched.  Each frame is read once; any byte
 * alignment of the frames.  EC_ERR_SHAPE unless 1 <= C <= 64, H >= 3, W >= 3, 1 <= B <= 65535. */
int ec_semantic_labels_u8(const uint8_t* sem_u8, const uint8_t* colors_u8, int64_t* presence, int64_t* localization,
                          int B, int H, int W, int C, ec_stream_t stream);


/* out[M, N] (fp32) = act(A[M, K] (bf16) @ W^T + bias), W an fp32 [N, K] matrix handed over as the three bf16 planes
 * ec_split3_bf16 writes ([N][3][K]): the exact-fp32 product of stored bf16 features with fp32 weights -- the first
 * 1x1 conv of ResnetTensorGoalEncoder.resnet_compressor (allenact_plugins/robothor_plugin/.../resnet_tensor encoders;
 * SURVEY.md section 8 row a) -- on the 8-wave ping-pong kernel.  N % 128 == 0, K % 64 == 0. */
int ec_split3_bf16(const float* W, void* planes, long rows, int K, ec_stream_t stream);
int ec_gemm_bf16a_x3(const void* A_bf16, const void* W_planes, const float* bias, float* out, long M, int N, int K,
                     int act, ec_stream_t stream);

/* dW[128, NX] += dY^T X over M token rows: dY as three bf16 planes [M][3][128] (ec_split3_bf16 layout), X bf16 [M][NX]
 * (NX % 256 == 0) -- the weight gradient of the compressor's first 1x1 conv over the stored features.  `part` is scratch
 * of ec_dw_tn_x3_splits(M, NX) * 128 * NX floats (per-split partial tiles, folded deterministically). */
int ec_dw_tn_x3_splits(long M, int NX);
int ec_dw_tn_x3(const void* dY_planes, const void* X_bf16, float* part, float* dW, long M, int NX, ec_stream_t stream);

/* Stem conv1: 3x3 stride 2 pad 1 on the fp32 NHWC frame the RGB sensor hands
 * over ([U] ClipResNetPreprocessor.process: obs[rgb].permute(0,3,1,2)), folded
 * BN + ReLU, LDS-staged image tiles.  w f32 [3*3*3][Cout] (ky,kx,ci major),
 * out bf16 [B,H/2,W/2,Cout].  Cout in {32,48}. */
int ec_stem_conv1(const float* rgb_nhwc, const float* w, const float* bias, void* out,
                  int B, int H, int W, int Cout, ec_stream_t stream);

/* Stem conv1 on a ONE-channel frame: the depth tower of the RGB-D agent (readme_files/baselines_habitat.md:75 "replace `rgb`
 * with `rgbd`"; [U] a second ClipResNetPreprocessor on the depth sensor, which repeats the frame to three channels).
 * depth f32 [B,H,W] (== [B,H,W,1]); the value fed to the conv is depth*scale + shift for pixels inside the frame and exactly 0
 * in the padding (zero in the NORMALISED domain, as ec_stem_conv1_u8 does); w9 f32 [9][Cout], tap-major (ky*3+kx),
 * w9[k][co] = sum_ci w[(k*3+ci)][co] of ec_stem_conv1's weights (the channel repeat folded in); bias f32 [Cout];
 * out bf16 NHWC [B,Ho,Wo,Cout], Ho = (H-1)/2+1.  3x3, stride 2, pad 1, folded BN + ReLU.  Cout in {32, 48, 64}: the two
 * arithmetic routes of ec_stem_conv1 (bf16 MFMA for 32 / 64 with the window K = 9 padded to 16, packed fp32 FMAs for 48).
 * Reads 4 B and writes Cout/2 B per input pixel: 200,704 B in, 802,816 B out per 224 x 224 frame at Cout = 64.
 * Checked before any HIP call: NULL -> EC_ERR_ARG; B <= 0, H < 2, W < 2 or another Cout -> EC_ERR_SHAPE. */
int ec_stem_conv1_depth(const float* depth, float scale, float shift, const float* w9, const float* bias, void* out,
                        int B, int H, int W, int Cout, ec_stream_t stream);

/* Fused pair of 1x1 convolutions across a Bottleneck boundary of layer1 (bandwidth-bound at 56x56):
 *   y = relu(a0 . w0^T + b0 [+ a1 . w1^T + b1] [+ res])   [M,256]  == relu(bn3(conv3(out)) + identity), the identity
 *                                                                    being `res` or the fused downsample conv (a1,w1,b1)
 *   z = relu(y . w2^T + b2)                               [M,N2]   == the next block's relu(bn1(conv1(x)))
 * ([U] openai/CLIP clip/model.py Bottleneck.forward; call site thor_image_features.py:109).
 * a0,a1 bf16 [M,64]; w0,w1 bf16 [256,64]; res,y bf16 [M,256]; w2 bf16 [N2,256]; z bf16 [M,N2].
 * K0 must be 64, N 256, N2 64 or 128 (64 only with a1), M a multiple of 32; else EC_ERR_SHAPE.
 * y may be NULL at these widths: it is not stored then (z is the same bits) -- for a caller whose next launch rebuilds y
 * (ec_conv1x1_pair_rebuild_bf16). */
int ec_conv1x1_pair_bf16(const void* a0, const void* w0, const float* b0, const void* a1, const void* w1,
                         const float* b1, const void* res, void* y, const void* w2, const float* b2, void* z,
                         long M, int K0, int N, int N2, ec_stream_t stream);

/* The NEXT boundary behind a ec_conv1x1_pair_bf16(a0 = i0, a1 = i1, res = NULL, y = NULL) launch: the identity is rebuilt from
 * that launch's inputs instead of being read from memory:
 *   id = relu(i0 . wi0^T + bi0 + i1 . wi1^T + bi1)        [M,256]  never stored; == the y of that launch, bit for bit
 *   y  = relu(a . w3^T + b3 + id)                         [M,256]  == relu(bn3(conv3(out)) + identity) of layer1.1
 *   z  = relu(y . w2^T + b2)                              [M,64]   == layer1.2's relu(bn1(conv1(x)))
 * ([U] openai/CLIP clip/model.py Bottleneck.forward; call site thor_image_features.py:109).  y and z are bit-identical to
 * ec_conv1x1_pair_bf16(a, w3, b3, res = id, ...).  a, i0, i1 bf16 [M,64]; w3, wi0, wi1 bf16 [256,64]; w2 bf16 [64,256].
 * Reads 384 B and writes 640 B per pixel (with the identity read from memory: 640 B and 640 B, and 512 B written in front).
 * NULL -> EC_ERR_ARG; M not a positive multiple of 32, K0 != 64, N != 256 or N2 != 64 -> EC_ERR_SHAPE. */
int ec_conv1x1_pair_rebuild_bf16(const void* a, const void* w3, const float* b3, const void* i0, const void* wi0,
                                 const float* bi0, const void* i1, const void* wi1, const float* bi1, void* y,
                                 const void* w2, const float* b2, void* z, long M, int K0, int N, int N2,
                                 ec_stream_t stream);

/* Same fused pair at the layer-1 -> layer-2 boundary (res given, N2 = 128), which ALSO emits y_pooled =
 * AvgPool2d(2)(y) bf16 [B, H/2, W/2, 256] -- the input of the next block's downsample path ([U] Bottleneck:
 * `downsample = Sequential(AvgPool2d(stride), Conv2d 1x1, BatchNorm2d)`) -- so that no separate pooling pass re-reads y.
 * Tiles are 4 x 8 pixel blocks: H % 4 == 0 and W % 8 == 0. */
int ec_conv1x1_pair_pool_bf16(const void* a0, const void* w0, const float* b0, const void* res, void* y,
                              void* y_pooled, const void* w2, const float* b2, void* z, int B, int H, int W, int K0,
                              int N, int N2, ec_stream_t stream);

/* Same, on the RAW uint8 HWC frame (thor_frames.py:33-34,96 writes uint8 frames): ToTensor (/255) and
 * Normalize(mean, std) of `clip_preprocess` (thor_image_features.py:108) are fused into the LDS staging.
 * h_mean3 / h_std3 are HOST pointers to 3 floats (CLIP_RGB_MEANS / CLIP_RGB_STDS). */
int ec_stem_conv1_u8(const uint8_t* rgb_u8_nhwc, const float* h_mean3, const float* h_std3, const float* w,
                     const float* bias, void* out, int B, int H, int W, int Cout, ec_stream_t stream);

/* Bottleneck-level fusion (conv_bneck.hip): conv2 (3x3) + bn2 + ReLU and conv3 (1x1) + bn3 + identity + ReLU of ONE
 * stride-1 Bottleneck in one launch, one workgroup per image, the image's 14 x 14 x C map resident in LDS -- replaces the
 * last two convs of [U] clip/model.py Bottleneck.forward for CLIP-RN50 layer3.1 .. layer3.5 (planes C = 256), reached
 * through `clip_model(clip_input)` (primitive_probing/generate_data/thor_image_features.py:109).
 * c1 bf16 [B,14,14,C] = relu(bn1(conv1(x))); b2 / b3 f32 (folded BatchNorm); x (identity) and y bf16 [B,14,14,4C].
 * The weights come in the kernel's streaming order: ec_bneck_pack_weights(w2 bf16 [C][3*3*C], w3 bf16 [4C][C]) ->
 * packed (ec_bneck_packed_elems(C) bf16 elements, conv2 then conv3; once per set of weights).
 * Bit-identical to ec_conv_bf16(3x3) followed by ec_conv_bf16(1x1, res = x).  EC_ERR_SHAPE unless H = W = 14, C = 256. */
size_t ec_bneck_packed_elems(int C);
int ec_bneck_pack_weights(const void* w2, const void* w3, void* packed, int C, ec_stream_t stream);
int ec_bneck_conv23_bf16(const void* c1, const void* packed, const float* b2, const float* b3,
                         const void* x, void* y, int B, int H, int W, int C, ec_stream_t stream);

/* The WHOLE stride-1 Bottleneck in one launch (conv1 + bn1 + ReLU in front of the two above; c1 never exists in HBM: the
 * block input x streams through a shared LDS ring): y = relu(conv3(relu(conv2(relu(conv1(x)))) + x).  packed =
 * ec_bneck3_pack_weights(w1 bf16 [C][4C], w2, w3) (ec_bneck3_packed_elems(C) elements).  Bit-identical to the three ec_conv_bf16
 * calls.  Same geometry restriction. */
size_t ec_bneck3_packed_elems(int C);
int ec_bneck3_pack_weights(const void* w1, const void* w2, const void* w3, void* packed, int C, ec_stream_t stream);
int ec_bneck_conv123_bf16(const void* x, const void* packed, const float* b1, const float* b2, const float* b3,
                          void* y, int B, int H, int W, int C, ec_stream_t stream);

/* relu(bn2(conv2(x))) of a late Bottleneck for SMALL launches (<= 64 frames: the per-GPU batches of strong scaling,
 * readme_files/baselines_habitat.md:63-73): one workgroup per (image, 32/64-channel slice), the image's map resident in
 * LDS, the eight waves split K and their partial tiles are folded through LDS in a fixed order (deterministic; equal to
 * ec_conv_bf16 up to fp32-accumulation rounding).  Geometries: (H = W = 14, C = 256), (H = W = 7, C = 512) and, with
 * pool = 1 (CLIP's anti-aliased stride: ReLU then AvgPool2d(2), out [B,7,7,C]; the 200-KB map resident in two channel
 * chunks), (H = W = 14, C = 512); else EC_ERR_SHAPE.  in / out bf16 [B,H,W,C]; packed = ec_conv3x3_img_pack(w bf16
 * [C][3*3*C]) (C * 9C elements). */
int ec_conv3x3_img_pack(const void* w, void* packed, int C, ec_stream_t stream);
int ec_conv3x3_img_bf16(const void* in, const void* packed, const float* bias, void* out, int B, int H, int W, int C,
                        int pool, ec_stream_t stream);
/* ... its pooled geometry with an output row stride (see ec_conv_bf16_ld); out_row_stride != C needs pool = 1. */
int ec_conv3x3_img_bf16_ld(const void* in, const void* packed, const float* bias, void* out, int B, int H, int W, int C,
                           int pool, int out_row_stride, ec_stream_t stream);

/* ------------------------------------------------------------------------
 * torchvision ResNet-50 pieces: the ImageNet half of the feature scripts,
 * `resnet_model = Sequential(*list(models.resnet50(pretrained=True).children())[:-2])`
 * (primitive_probing/generate_data/thor_image_features.py:46-49,102-106; reachable_image_features.py:48-51,81-85).
 * ---------------------------------------------------------------------- */
/* Stride-2 convolution (1x1, or 3x3 with pad 1) + folded BatchNorm (+ residual) + activation: ResNet v1.5 strides
 * inside Bottleneck.conv2 and in the downsample conv, where CLIP's ModifiedResNet pools.  in bf16 [B,H,W,Cin] (H, W
 * even); w bf16 [Cout][k*k*Cin]; res / out bf16 [B,H/2,W/2,Cout].  Cin % 8 == 0, Cout % 64 == 0; act NONE or RELU. */
int ec_conv_bf16_s2(const void* in, const void* w, const float* bias, const void* res, void* out, int B, int H, int W,
                    int Cin, int Cout, int ksize, int act, ec_stream_t stream);
/* torchvision BasicBlock transition tail (ResNet-18 / 34, first block of layers 2-4) in ONE launch:
 *   out = relu(conv3x3(c1) + conv1x1_stride2(x) + bias_cat)
 * as one implicit GEMM over K = 9*planes + inplanes (conv_basic.hip).  c1 bf16 [B,Ho,Wo,planes] (conv1's output),
 * x bf16 [B,2Ho,2Wo,inplanes] (the block input), w_cat bf16 [Cout][9*planes + inplanes] = [conv2 (ky,kx,ci) | downsample
 * (ci)] with BN folded, bias_cat f32 [Cout] = b2 + bd; out bf16 [B,Ho,Wo,Cout], rounded once.  planes, inplanes and
 * Cout are multiples of 64.  Replaces conv2 + bn2 + downsample + `out += identity` + relu of [U] torchvision
 * models/resnet.py BasicBlock.forward. */
int ec_basic_tail_s2_bf16(const void* c1, const void* x, const void* w_cat, const float* bias_cat, void* out, int B, int Ho,
                          int Wo, int planes, int inplanes, int Cout, ec_stream_t stream);
/* conv1 (7x7, stride 2, pad 3, 3 -> 64) + bn1 (folded) + ReLU + MaxPool2d(3, 2, 1) in one launch (the conv output never
 * touches HBM).  rgb: fp32 NHWC [B,H,W,3], ImageNet-normalised (u8 == 0), or raw uint8 NHWC with ToTensor +
 * Normalize(mean, std) of `resnet_preprocess` (thor_image_features.py:36-44) fused (u8 == 1; h_mean3 / h_std3 HOST
 * pointers to 3 floats).  w bf16 [64][176]: K = 7 rows (ky) of 24 slots, slot kx*3+ci < 21 real, the rest and the
 * last 8 zero; bias f32 [64]; out bf16 [B,H/4,W/4,64].  H, W multiples of 4. */
int ec_stem7_pool(const void* rgb, int u8, const float* h_mean3, const float* h_std3, const void* w, const float* bias,
                  void* out, int B, int H, int W, ec_stream_t stream);

/* AvgPool2d(2) on bf16 NHWC ([U] Bottleneck downsample "-1"). C multiple of 8. */
int ec_avgpool2_bf16(const void* in, void* out, int B, int H, int W, int C, ec_stream_t stream);
/* ... writing a column block of a wider tensor: pooled pixel q goes to out + q * out_row_stride (elements; see
 * ec_conv_bf16_ld).  `out` 16-B aligned. */
int ec_avgpool2_bf16_ld(const void* in, void* out, int B, int H, int W, int C, int out_row_stride, ec_stream_t stream);

/* bf16 NHWC [B,HW,C] -> fp32 NCHW [B,C,HW]: the `.float()` + layout the
 * reference exposes (thor_image_features.py:111; observation_space (2048,7,7)). */
int ec_nhwc_bf16_to_nchw_f32(const void* in, float* out, int B, int HW, int C, ec_stream_t stream);
/* The inverse for a consumer that holds the reference's fp32 NCHW tensors ([U] ResnetTensorObjectNavActorCritic.forward's
 * observations): fp32 [B,C,HW] -> bf16 [B,HW,C]; *inexact (device int, zeroed by the caller) is OR-ed with 1 when some
 * value is not exactly representable in bf16 -- the caller then keeps its fp32 path.  C % 64 == 0. */
int ec_nchw_f32_to_nhwc_bf16(const float* in, void* out, int B, int HW, int C, int* inexact, ec_stream_t stream);
/* ... for two tensors of one shape in ONE launch ([U] ai2thor-rearrangement ResNetRearrangeActorCriticRNN.forward's two
 * observations, the current and the unshuffled view, on every act step): a, b fp32 [B, C, HW].
 * out_a, out_b bf16 [B, HW, C]: round to nearest even.  *changed (device int) is set to 1 if any
 * non-NaN element of either input is not already a bf16 value; it is never cleared by the call
 * (sticky: the caller zeroes it).
 * Checked before any HIP call: a, b, out_a, out_b or changed NULL or not 16-byte aligned -> EC_ERR_ARG; B <= 0, HW outside
 * 1..64 or C % 64 != 0 -> EC_ERR_SHAPE. */
int ec_nchw_f32_pair_to_nhwc_bf16(const float* a, const float* b, void* out_a, void* out_b, long B,
                                  int HW, int C, int* changed, ec_stream_t stream);

/* AdaptiveAvgPool2d(1)+Flatten on the fp32-cast features
 * (thor_image_features.py:63-66,113; preprocessor pool=True). bf16 [B,HW,C] -> f32 [B,C]. */
int ec_spatial_mean_bf16(const void* in, float* out, int B, int HW, int C, ec_stream_t stream);
/* [U] ResNetCLIPEncoder.forward, rgb + depth (habitat branch; restated, parity unpinned):
 * adaptive_avg_pool2d(a + b, 1).flatten(1) on the fp32-cast maps.
 * a, b bf16 [B,HW,C]; out f32 [B,C]; out[n,c] = (1/HW) * sum_hw (float(a[n,hw,c]) + float(b[n,hw,c])).
 * Every C >= 1: 16-byte loads when C % 8 == 0 and a, b are 16-byte aligned, 2-byte loads otherwise.  The summation order is
 * fixed (no float atomics): two calls give equal bits.  Checked before any HIP call: NULL -> EC_ERR_ARG; B, HW or
 * C <= 0 -> EC_ERR_SHAPE. */
int ec_spatial_mean_pair_bf16(const void* a, const void* b, float* out, int B, int HW, int C, ec_stream_t stream);

/* ------------------------------------------------------------------------
 * CLIP ModifiedResNet trunk (stem + layer1..4, attnpool detached):
 * `clip_model.visual` with `attnpool = Identity` (thor_image_features.py:59-67,109)
 * == [U] ClipResNetEmbedder.forward.
 * ---------------------------------------------------------------------- */
typedef struct ec_rn50 ec_rn50_t;

/* Weight order contract (execution order): stem conv1 (f32, [27][sc]) is
 * passed separately; `w_bf16` holds, concatenated, stem conv2, conv3, then per
 * block conv1, conv2, conv3, [downsample] as [Cout][k*k*Cin] bf16;
 * `bias` holds stem conv1..3 then the same per-block order, f32.
 * `width` is a multiple of 32 (64 = RN50, 96 = RN50x16).  The stem's w/2 channels are carried at
 * sc = roundup(w/2, 32) (RN50x16: 48 -> 64): stem conv1 is [27][sc], conv2 [sc][9*sc], conv3 [w][9*sc], with zero
 * weights / biases in the padding (exactly neutral after ReLU).
 * The handle borrows the device pointers (caller keeps them alive). */
int ec_rn50_create(ec_rn50_t** out, int width, const int* layers4, int input_resolution,
                   const float* stem_w_f32, const void* w_bf16, size_t n_w, const float* bias, size_t n_bias);
/* The torchvision ResNet trunk (width 64) behind the same handle type: every ec_rn50_* function below applies.
 * stem_w_bf16 = conv1 in ec_stem7_pool's layout; `w_bf16` / `bias` hold per block conv1, conv2, conv3, [downsample]
 * (bias: stem first) exactly as for ec_rn50_create.  ec_rn50_forward takes the ImageNet-normalised fp32 frame,
 * ec_rn50_forward_u8 the raw frame + IMAGENET mean / std.  Output bf16 NHWC [B,R/32,R/32,2048] == `imagenet_conv`
 * (thor_image_features.py:105,130) before its `.float()` / NCHW view. */
int ec_rn50tv_create(ec_rn50_t** out, const int* layers4, int input_resolution, const void* stem_w_bf16,
                     const void* w_bf16, size_t n_w, const float* bias, size_t n_bias);
/* The torchvision BasicBlock ResNet trunk (ResNet-18: layers4 = 2,2,2,2; ResNet-34: 3,4,6,3) behind the same handle
 * type: every ec_rn50_* function below applies.  stem_w_bf16 as for ec_rn50tv_create; `w_bf16` / `bias` hold per block
 * conv1, conv2, [downsample] (bias: stem first), BN folded.  ResNet-18 at 224: 11,157,504 weights + the stem's 9,408,
 * 4,800 biases.  Output bf16 NHWC [B,R/32,R/32,512] == `Sequential(*list(resnet18().children())[:-2])` before the
 * NCHW view ([U] allenact embodiedai/preprocessors/resnet.py ResNetEmbedder with pool=False). */
int ec_tvresnet_basic_create(ec_rn50_t** out, const int* layers4, int input_resolution, const void* stem_w_bf16,
                             const void* w_bf16, size_t n_w, const float* bias, size_t n_bias);
void ec_rn50_destroy(ec_rn50_t* h);
size_t ec_rn50_workspace_bytes(const ec_rn50_t* h, int batch);
int ec_rn50_out_channels(const ec_rn50_t* h);
int ec_rn50_out_spatial(const ec_rn50_t* h);
/* rgb f32 NHWC [B,R,R,3] -> feat bf16 NHWC [B,R/32,R/32,32w].  `feat` may be a
 * slice of the rollout feature buffer.  chunk>0 runs the trunk in sub-batches
 * of `chunk` frames so intermediates stay Infinity-Cache resident. */
int ec_rn50_forward(const ec_rn50_t* h, const float* rgb_nhwc, int batch, void* workspace, size_t ws_bytes,
                    void* feat_bf16_nhwc, int chunk, ec_stream_t stream);
/* uint8 frames in (fused input pipeline; 4x fewer input bytes, no fp32 frame tensor). */
int ec_rn50_forward_u8(const ec_rn50_t* h, const uint8_t* rgb_u8_nhwc, const float* h_mean3, const float* h_std3,
                       int batch, void* workspace, size_t ws_bytes, void* feat_bf16_nhwc, int chunk,
                       ec_stream_t stream);
/* The depth tower of the RGB-D agent: ec_rn50_forward's plan with the stem's first conv served by ec_stem_conv1_depth.
 * depth f32 [B,R,R] (== [B,R,R,1]), normalised as depth*scale + shift inside the kernel; stem_w9 f32 [9][stem channels]
 * (device; see ec_stem_conv1_depth) is passed per call -- the handle stays pointer-only and both towers of the agent read
 * the same frozen weights, as [U] AllenAct's two preprocessors do.  `chunk` as above.  A handle of the torchvision towers
 * (7x7 stem) returns EC_ERR_UNSUPPORTED; NULL pointers EC_ERR_ARG. */
int ec_rn50_forward_depth(const ec_rn50_t* h, const float* depth, float scale, float shift, const float* stem_w9, int batch,
                          void* workspace, size_t ws_bytes, void* feat_bf16_nhwc, int chunk, ec_stream_t stream);
/* The RGB-D encoder of the Habitat DD-PPO net ([U] habitat branch ResNetCLIPEncoder with rgb and depth; restated, parity
 * unpinned): the trunk on the RGB frame and on the depth frame of every pair, the two maps summed and average-pooled:
 * embed f32 [pairs, out_channels] = adaptive_avg_pool2d(trunk(rgb) + trunk(depth), 1).flatten(1).  Replaces two trunk forwards,
 * the add and the pool.  Both towers read the same weights, so a chunk of nb pairs is ONE pass of ec_rn50_forward's plan at
 * 2 nb frames: the stem's first conv is two launches into one buffer (ec_stem_conv1 / _u8 on rows [0, nb), ec_stem_conv1_depth on
 * rows [nb, 2 nb)), every later op runs once, and ec_spatial_mean_pair_bf16 ends the chunk.  EC_RGBD_JOINT=0: two passes at nb
 * frames (RGB, then depth) and the same pool.
 * rgb f32 or (rgb_u8 != 0) uint8 [pairs,R,R,3], the latter with host mean / std as ec_rn50_forward_u8; depth, scale, shift,
 * stem_w9 as ec_rn50_forward_depth.  `pairs` and `chunk` count PAIRS.  workspace: ec_rn50_rgbd_workspace_bytes(h, chunk) --
 * the plan's buffers at 2 * chunk frames plus the chunk's maps.  Checked before the first launch: NULL rgb, depth, stem_w9,
 * workspace or embed (h_mean3 / h_std3 with rgb_u8) -> EC_ERR_ARG; pairs <= 0 -> EC_ERR_SHAPE; a handle of the torchvision towers
 * (7x7 stem) -> EC_ERR_UNSUPPORTED; a short workspace -> EC_ERR_WORKSPACE. */
size_t ec_rn50_rgbd_workspace_bytes(const ec_rn50_t* h, int pairs);
int ec_rn50_embed_rgbd(const ec_rn50_t* h, const void* rgb, int rgb_u8, const float* h_mean3, const float* h_std3,
                       const float* depth, float scale, float shift, const float* stem_w9, int pairs, void* workspace,
                       size_t ws_bytes, float* embed, int chunk, ec_stream_t stream);
/* Number of ops in the handle's launch plan (from 128 frames on one kernel launch each: 38 for CLIP RN50 at 224 x 224;
 * smaller launches run the five fused layer-3 blocks as three launches each).  Tests and tools/ key on it. */
int ec_rn50_num_ops(const ec_rn50_t* h);
/* 64-bit hash of the handle's launch plan (op kinds, shapes, buffer routing) and the library version: identifies
 * what a profiler summary under profiles/ was measured on (bench.py rejects a stale one). */
uint64_t ec_rn50_plan_hash(const ec_rn50_t* h);
/* Tuning property of the handle (no reference counterpart): fewest 256-row output tiles for which this trunk's conv
 * launches take the 8-wave kernel (0 = library default, 150).  A caller that keeps two encoder launches in flight on
 * two streams (engine.Worker with 128-frame slices) sets 50 on both handles: each launch then occupies fewer, fully
 * used CUs.  Part of the plan hash; affects only this handle's forwards (it is not process state). */
int ec_rn50_set_conv8_min_tiles(ec_rn50_t* h, int n);
/* Tuning property of the handle (no reference counterpart), off by default: layer 1's block-0 output -- 512 B per pixel written
 * by the layer1.0 boundary launch and read back once as the identity of layer1.1 -- is not stored; the layer1.1 boundary launch
 * rebuilds it from block 0's conv2 output and block input (ec_conv1x1_pair_rebuild_bf16).  Same number of launches, features
 * bit-identical, 768 B per 56 x 56 pixel less HBM traffic.  Accepted only on a CLIP tower whose layer1.0 and layer1.1 boundaries
 * run as fused pairs (width 64, layer 1 of at least three blocks, EC_RN50_FUSE on); EC_ERR_UNSUPPORTED otherwise, and the handle
 * is unchanged.  The plan is rebuilt (same workspace size); part of the plan hash only while on.  Not to be called while a
 * forward of this handle is being issued. */
int ec_rn50_set_l1_rebuild(ec_rn50_t* h, int on);


/* ------------------------------------------------------------------------
 * General fp32 GEMM on the exact-fp32 MFMA:  C (+)= epi(A B),
 * A(m,k) = A[m*sam + k*sak], B(k,n) = B[k*sbk + n*sbn]  (NT / NN / TN by strides).
 * Replaces the cuBLAS calls behind nn.Conv2d(1x1) / nn.Linear / nn.GRU and their
 * autograd backward in the policy ([U] allenact ResnetTensorGoalEncoder,
 * RNNStateEncoder, LinearActorHead/CriticHead).
 * Epilogue order: + bias[n] + gbias[gidx[m/group]][n] -> relu -> * rowscale[m]
 * -> * (dmask[m,n] > 0) -> store / += / atomicAdd (splitk > 1; C pre-initialised).
 * ---------------------------------------------------------------------- */
enum {
    EC_GEMM_A_BF16 = 1,      /* A stored as bf16 (the frozen CLIP features) */
    EC_GEMM_B_BF16 = 2,
    EC_GEMM_RELU = 4,
    EC_GEMM_ACCUMULATE = 8,  /* C += ... */
    EC_GEMM_SPLIT_PARTS = 16,/* splitk > 1: slice z writes its partial sums to C + z * M * ldc (no atomics; the caller folds
                              * the parts in a fixed order); bias goes into part 0; no ReLU / mask / row scale */
    EC_GEMM_3PRODUCTS = 32   /* bf16x3 path: only the three leading bf16 products a0 b0 + a0 b1 + a1 b0 of an fp32 x fp32 product
                              * (relative error 2^-16 per product instead of 2^-24; half the MFMAs).  Meant for GRADIENT GEMMs
                              * (ec_policy_backward with EC_GEMM_BWD3=1); ignored on the exact-fp32 MFMA path */
};
int ec_gemm_f32(const void* A, const void* B, float* C, int M, int N, int K, long sam, long sak, long sbk, long sbn,
                int ldc, int flags, const float* bias, const float* gbias, const int* gidx, int group,
                const float* dmask, const float* rowscale, int splitk, ec_stream_t stream);

/* ------------------------------------------------------------------------
 * GRU actor-critic policy == ActorCriticModel.forward as
 * ResnetTensorObjectNavActorCritic ([U] allenact; launched by
 * readme_files/baselines_robothor_objectnav.md:48-51) and its backward.
 * params/grads: ONE flat fp32 buffer each, tensors in AllenAct order
 * (embed_class, compressor.0.{w,b}, compressor.2.{w,b}, combiner.0.{w,b},
 * combiner.2.{w,b}, rnn.weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0,
 * actor.linear.{w,b}, critic.fc.{w,b}) at ec_policy_param_offset() (16-B aligned).
 * ---------------------------------------------------------------------- */
typedef struct {
    int in_channels;   /* 2048 */
    int spatial;       /* 7    */
    int hidden;        /* 512  */
    int goal_dims;     /* 32   */
    int num_goals;     /* 12   */
    int num_actions;   /* 6    */
    int compress_hid;  /* 128  */
    int compress_out;  /* 32   */
    int comb_hid;      /* 128  */
    int comb_out;      /* 32   */
    int fusion;        /* 0: ResnetTensorGoalEncoder (goal-embedding fusion of the RoboTHOR/Habitat configs);
                        * 1: zero-shot dual-encoder fusion (readme_files/zeroshot_objectnav.md:3-8; builder-defined,
                        *    parity-unpinned): x = feat/|feat| (*) goal_table[goal], feat = [T*N, 1, in_channels] CLIP
                        *    image embeddings, goal_table = frozen CLIP text embeddings (ec_policy_set_goal_table);
                        *    spatial must be 1, the compressor/combiner fields are ignored and those nine parameter
                        *    tensors have zero elements (the trainable part is GRU + heads) */
    int dual;          /* 1: RGB + depth, [U] ResnetDualTensorGoalEncoder (readme_files/baselines_habitat.md:75 "replace rgb
                        *    with rgbd"): two feature tensors, each with its own compressor / combiner (the goal embedding is
                        *    shared), rgb_x and depth_x concatenated along channels before nn.Flatten -> GRU input
                        *    2 * comb_out * spatial^2.  Eight more parameter tensors (the depth stream's, after the 17 of
                        *    the single encoder); use ec_policy_forward2 / ec_policy_backward2.  Not combinable with fusion */
    int goal_in;       /* 0: the goal of a frame is an integer id (embed_class, the ObjectNav models above).
                        * k in 1..8: the goal of a frame is k floats (PointNav: polar (rho, phi) from the GPS + compass sensor,
                        *    k = 2; Habitat's own policy feeds (rho, cos -phi, sin -phi), k = 3) through
                        *    embed_goal = nn.Linear(k, goal_dims) -- [U] allenact ~v0.5.0 projects/pointnav_baselines/models/
                        *    point_nav_models.py ResnetTensorPointNavActorCritic, restated from the published source (parity
                        *    unpinned, like the rest of the policy).  num_goals is ignored.  18 parameter tensors:
                        *    embed_goal.weight [goal_dims, k] and embed_goal.bias [goal_dims] first, then the 16 others of the
                        *    single encoder in the order above.  Use ec_policy_forward_vec / ec_policy_act_vec; the backward
                        *    entry points are the same.  EC_ERR_ARG with fusion = 1; EC_ERR_UNSUPPORTED with dual = 1 (the
                        *    RGB-D PointNav encoder is not built) */
    int prev_action_dims;  /* E.  0: the GRU reads the goal encoder's output alone -- today's handle exactly (tensor count, flat
                        *    size, workspace sizes, launch plan and bits).
                        * E in 1..64: the embedding of the previous action is concatenated to the GRU input ([U] habitat_baselines
                        *    PointNavResNetPolicy prev_action_embedding, width 32; [U] allenact VisualNavActorCritic
                        *    add_prev_actions / action_embed_size, default 6) -- restated from the published sources, parity
                        *    unpinned.  rnn.weight_ih_l0 becomes [3 * hidden, flat + E] (one tensor; flat = today's input width)
                        *    and ONE more tensor, prev_action_embedder.fc.weight [num_actions + prev_action_null, E], is the
                        *    last of the flat order.  Nothing [T*N, E]-shaped exists: the embedding reaches gi through the
                        *    weight-derived table of ec_prev_action_table (built with the other tables: per EC_POLICY_INFER
                        *    call, kept under EC_POLICY_INFER_REUSE, per learn pass).  No GEMM reads weight_ih in place on
                        *    such a handle (its row stride need not be a multiple of 4): every route goes through a dense
                        *    [3 * hidden, flat] copy, and the dense gradient is added back row by row.  Use ec_policy_forward_pa /
                        *    ec_policy_act_pa; the backward entry points are the same.  EC_ERR_ARG outside 0..64;
                        *    EC_ERR_UNSUPPORTED with dual = 1 or fusion = 1 (like goal_in with dual: the two-tower and the
                        *    zero-shot agents with previous actions are not built) */
    int prev_action_null;  /* 1: row 0 of the embedding is the null token of an episode's first step (masks == 0) and action a is
                        *    row a + 1 (Habitat; allenact add_prev_action_null_token); 0: action a is row a.  EC_ERR_ARG outside
                        *    {0, 1} and with prev_action_dims == 0 */
} ec_policy_cfg;
typedef struct ec_policy ec_policy_t;

int ec_policy_create(ec_policy_t** out, const ec_policy_cfg* cfg);
/* The recurrent cell ([U] allenact RNNStateEncoder(input, hidden, num_layers=1, rnn_type="GRU" | "LSTM"); the Habitat DD-PPO
 * policies of readme_files/baselines_habitat.md:63-73 are LSTM policies).  ec_policy_create(out, cfg) ==
 * ec_policy_create_rnn(out, cfg, EC_RNN_GRU): that handle is today's, bit for bit.  EC_RNN_LSTM: torch.nn.LSTM's cell under the
 * episode mask, which resets BOTH states (restated from the published sources, parity unpinned):
 *   hp = m*h_prev; cp = m*c_prev;  a = W_ih x + b_ih + W_hh hp + b_hh  (gate order i, f, g, o: rows 0..H-1, H..2H-1, ...)
 *   i = s(a_i); f = s(a_f); g = tanh(a_g); o = s(a_o);  c = f*cp + i*g;  h = o*tanh(c)
 * The same tensor names in the same order; rnn.weight_ih_l0 is [4H, flat (+E)], weight_hh_l0 [4H, H], both biases [4H].
 * The recurrent state of an actor is ONE row [h | c] of width 2H (ec_policy_state_width): on an LSTM handle every h0, h_final
 * and dh_final of the entry points below is f32 [N, 2H] where the comments say [N,H], and ec_policy_workspace_bytes grows by
 * the cell-state history and the fourth gate.  Every entry point keeps its signature.  No float atomics on any route of an
 * LSTM handle: two learn passes give equal bits, and an actor's result does not depend on how the actors are sliced.
 * EC_ERR_ARG for any other rnn_type; EC_ERR_UNSUPPORTED for EC_RNN_LSTM with dual = 1 or fusion = 1 (the two-tower and the
 * zero-shot agents keep the GRU); EC_ERR_SHAPE unless hidden % 32 == 0 (and hidden % 256 == 0 or hidden <= 608: the forward
 * step's two operand tiles sit in LDS). */
enum { EC_RNN_GRU = 0, EC_RNN_LSTM = 1 };
int ec_policy_create_rnn(ec_policy_t** out, const ec_policy_cfg* cfg, int rnn_type);
int ec_policy_rnn_type(const ec_policy_t* h);          /* EC_RNN_GRU | EC_RNN_LSTM (-1: NULL handle) */
int ec_policy_state_width(const ec_policy_t* h);       /* L * (H (GRU) or 2H (LSTM)): the width of a row of h0 / h_final / dh_final */
/* Recurrent depth ([U] allenact RNNStateEncoder(.., num_layers = L, ..); the published Habitat DD-PPO configs say
 * num_recurrent_layers: 2): torch.nn.GRU / torch.nn.LSTM with num_layers = L (1..EC_RNN_MAX_LAYERS) and dropout = 0 under the
 * episode mask.  Layer 0 is the single-layer handle's; layer l >= 1 at step t takes x = h^{l-1}_t against weight_ih_l{l} [G,H],
 * weight_hh_l{l} [G,H], bias_ih_l{l} [G], bias_hh_l{l} [G] (G = 3H | 4H).  The mask multiplies the previous state (h, and c on an
 * LSTM handle) of EVERY layer and never a layer's input; the heads read the top layer's h.
 *   ec_policy_create_rnn(out, cfg, t) == ec_policy_create_rnn_layers(out, cfg, t, 1): plan, workspace sizes, launches and bits of
 *   that handle are unchanged.  EC_ERR_ARG outside 1..EC_RNN_MAX_LAYERS; EC_ERR_UNSUPPORTED for num_layers > 1 with dual = 1 or
 *   fusion = 1.
 * State: an actor's state stays ONE row of width L * SW (SW = H | 2H), layer-major -- [h^0 | h^1 | ...] on a GRU handle,
 *   [h^0 | c^0 | h^1 | c^1 | ...] on an LSTM handle; layer l's state is the slice at l * SW.  Every h0, h_final and dh_final of the
 *   entry points below is f32 [N, L*SW] where the comments say [N,H]; every entry point keeps its signature.
 * Tensors: the upper layers' four tensors each END the flat order (layer 1, 2, 3; weight_ih, weight_hh, bias_ih, bias_hh), behind
 *   prev_action_embedder.fc.weight where that exists: every tensor of the single-layer handle keeps its index and offset.
 * Act step (T = 1 inference): ONE launch per layer (rnn_stack.hip: input projection, recurrent projection and cell together;
 *   EC_RNN_STACK=0 in the environment: the general route); it needs h_final != h0, else -- and for every T > 1 pass -- the layers
 *   run one after the other, each with the single-layer step kernels and one GEMM for the next layer's input projection.  The
 *   backward runs from the top layer down.  No float atomics on any route of a handle with L > 1: two learn passes give equal
 *   bits, and an actor's result does not depend on how the actors are sliced. */
#define EC_RNN_MAX_LAYERS 4
int ec_policy_create_rnn_layers(ec_policy_t** out, const ec_policy_cfg* cfg, int rnn_type, int num_layers);
int ec_policy_rnn_layers(const ec_policy_t* h);        /* L (0: NULL handle) */
/* fusion == 1 only: borrow the device goal table f32 [num_goals, in_channels] (e.g. ec_text_forward over the goal
 * prompts, L2-normalised); frozen -- it receives no gradient. */
int ec_policy_set_goal_table(ec_policy_t* h, const float* table);
void ec_policy_destroy(ec_policy_t* h);
int ec_policy_num_param_tensors(const ec_policy_t* h);
size_t ec_policy_flat_size(const ec_policy_t* h);                      /* floats, incl. alignment padding */
int ec_policy_param_offset(const ec_policy_t* h, int idx, size_t* off, size_t* numel);
size_t ec_policy_workspace_bytes(const ec_policy_t* h, int T, int N, int for_backward);
/* feat [T*N, S*S, C] NHWC (bf16 if feat_bf16 else f32); goal int64 [T*N]; h0 f32 [N,H] (LSTM handle: [N,2H] rows [h | c]);
 * masks f32 [T*N] (h -- on an LSTM handle h and c -- is multiplied by masks[t] before step t: episode reset);
 * hv f32 [T*N, A+1] out: logits in cols 0..A-1, value in col A; h_final f32 [N,H] (LSTM handle: [N,2H]) or NULL.
 * for_backward (the kernel plan depends on this flag alone, never on the size of the buffer handed in):
 *   EC_POLICY_LEARN (1)        the workspace (ec_policy_workspace_bytes(.., 1)) keeps every activation ec_policy_backward needs;
 *                              with more than 7 actions also both heads as one packed [A + 1, H] table and its gradient (one GEMM
 *                              each way; no float atomics on any route of such a handle: two learn passes give equal bits);
 *   EC_POLICY_INFER (0)        inference only (act step; a workspace of ec_policy_workspace_bytes(.., 0) suffices);
 *   EC_POLICY_INFER_REUSE (2)  inference, and the weight-derived tables an EC_POLICY_INFER call left in THIS workspace are
 *                              still valid (unchanged parameters: the later act steps of a rollout) -- they are not rebuilt. */
enum { EC_POLICY_INFER = 0, EC_POLICY_LEARN = 1, EC_POLICY_INFER_REUSE = 2 };
int ec_policy_forward(const ec_policy_t* h, const float* params, const void* feat, int feat_bf16,
                      const int64_t* goal, const float* h0, const float* masks, int T, int N,
                      void* workspace, size_t ws_bytes, int for_backward, float* hv, float* h_final, ec_stream_t stream);
/* dual == 1: feat = the RGB preprocessor's features, feat2 = the depth preprocessor's (same shape and dtype); with
 * dual == 0 feat2 is ignored (ec_policy_forward == ec_policy_forward2 with feat2 = NULL). */
int ec_policy_forward2(const ec_policy_t* h, const float* params, const void* feat, const void* feat2, int feat_bf16,
                       const int64_t* goal, const float* h0, const float* masks, int T, int N,
                       void* workspace, size_t ws_bytes, int for_backward, float* hv, float* h_final, ec_stream_t stream);
/* The act step in ONE call ([U] allenact OnPolicyRLEngine.act: `actor_critic(...)`, then `distributions.sample()` and
 * `log_probs(actions)`): ec_policy_forward2 with T = 1 and EC_POLICY_INFER (reuse_tables = 0) / EC_POLICY_INFER_REUSE (1), whose
 * heads launch also samples -- actions int64 [N], logp f32 [N], values f32 [N] or NULL, keyed as in ec_sample_actions (h0, h_final:
 * [N,H], on an LSTM handle [N,2H] -- there the step kernel stores h for the heads and the [h | c] row: as many launches).  Bit-for-bit
 * the results of ec_policy_forward2 followed by ec_sample_actions; one launch less on the act step's serial chain.
 * EC_ERR_UNSUPPORTED for more than 7 actions (use the two calls). */
int ec_policy_act(const ec_policy_t* h, const float* params, const void* feat, const void* feat2, int feat_bf16,
                  const int64_t* goal, const float* h0, const float* masks, int N, void* workspace, size_t ws_bytes,
                  int reuse_tables, float* hv, float* h_final, int64_t* actions, float* logp, float* values,
                  uint64_t seed, uint64_t step, int first_actor, ec_stream_t stream);
/* goal_in > 0 handles: ec_policy_forward2 / ec_policy_act with the goal of every frame as goal_in floats, goal_vec f32
 * [T*N, goal_in].  The goal half of target_obs_combiner.0 is a PER-FRAME bias row E1f[b] = (goal_vec[b] Wc^T + bc) W3[:, co:]^T + b3
 * that every call rebuilds from ITS goal vectors: EC_POLICY_INFER_REUSE keeps weight-derived tables only (the re-ordered
 * weight_ih, W1's planes), never a goal.  A learn pass leaves the goal vectors and their embeddings in the workspace for
 * ec_policy_backward*.  No float atomics anywhere on these handles: two runs give the same bits, and an actor's result does
 * not depend on how the actors are sliced.  The integer-goal entry points return EC_ERR_ARG on a goal_in > 0 handle, these
 * on a goal_in == 0 handle. */
int ec_policy_forward_vec(const ec_policy_t* h, const float* params, const void* feat, const void* feat2, int feat_bf16,
                          const float* goal_vec, const float* h0, const float* masks, int T, int N,
                          void* workspace, size_t ws_bytes, int for_backward, float* hv, float* h_final, ec_stream_t stream);
int ec_policy_act_vec(const ec_policy_t* h, const float* params, const void* feat, const void* feat2, int feat_bf16,
                      const float* goal_vec, const float* h0, const float* masks, int N, void* workspace, size_t ws_bytes,
                      int reuse_tables, float* hv, float* h_final, int64_t* actions, float* logp, float* values,
                      uint64_t seed, uint64_t step, int first_actor, ec_stream_t stream);
/* The EVALUATION act step (the reference's readme_files/baselines_robothor_objectnav.md:66-68 `--eval`,
 * baselines_habitat.md:89-97 `--run-type eval`, zeroshot_objectnav.md:20-27 `--eval -c $CKPT_PATH`): ec_policy_act /
 * ec_policy_act_vec whose heads launch takes [U] CategoricalDistr.mode() -- the FIRST index of the maximal logit -- instead of
 * a draw; logp = log_prob(actions) with the normaliser of the sampling route.  No seed, step or actor key: nothing is drawn.
 * hv and h_final are those of ec_policy_forward2 / _vec; actions, logp, values are those of ec_mode_actions on that hv, bit
 * for bit.  Same error codes as ec_policy_act (EC_ERR_UNSUPPORTED for more than 7 actions: use the two calls). */
int ec_policy_act_greedy(const ec_policy_t* h, const float* params, const void* feat, const void* feat2, int feat_bf16,
                         const int64_t* goal, const float* h0, const float* masks, int N, void* workspace, size_t ws_bytes,
                         int reuse_tables, float* hv, float* h_final, int64_t* actions, float* logp, float* values,
                         ec_stream_t stream);
int ec_policy_act_vec_greedy(const ec_policy_t* h, const float* params, const void* feat, const void* feat2, int feat_bf16,
                             const float* goal_vec, const float* h0, const float* masks, int N, void* workspace, size_t ws_bytes,
                             int reuse_tables, float* hv, float* h_final, int64_t* actions, float* logp, float* values,
                             ec_stream_t stream);
/* dhv f32 [T*N, A+1] = dLoss/dhv; dh_final [N,H] (LSTM handle: [N,2H] rows [dL/dh | dL/dc]) or NULL; grads += dLoss/dparams.
 * `workspace` must be the one the matching ec_policy_forward filled (for_backward size). */
int ec_policy_backward(const ec_policy_t* h, const float* params, const void* feat, int feat_bf16,
                       const float* masks, int T, int N, void* workspace, size_t ws_bytes, const float* dhv,
                       const float* dh_final, float* grads, ec_stream_t stream);
int ec_policy_backward2(const ec_policy_t* h, const float* params, const void* feat, const void* feat2, int feat_bf16,
                        const float* masks, int T, int N, void* workspace, size_t ws_bytes, const float* dhv,
                        const float* dh_final, float* grads, ec_stream_t stream);
/* ec_policy_backward2 that also records `recurrent_grads_ready` (a hipEvent_t, or NULL) on `stream` at the point where the
 * gradients of rnn.weight_ih_l0 ... critic.fc.bias (one contiguous section of the flat bucket, 92 % of its bytes) are final
 * and only the goal encoder's remain to be written: the data-parallel caller starts that section's SUM all-reduce behind the
 * event, under the rest of the backward.  Replaces the `async_op=True` per-parameter all-reduces of [U] allenact
 * OnPolicyTrainer.backprop_step (§8e "can be fully overlapped with the GRU-backward tail"). */
int ec_policy_backward3(const ec_policy_t* h, const float* params, const void* feat, const void* feat2, int feat_bf16,
                        const float* masks, int T, int N, void* workspace, size_t ws_bytes, const float* dhv,
                        const float* dh_final, float* grads, ec_event_t recurrent_grads_ready, ec_stream_t stream);

/* The LSTM step alone (lstm.hip; what the two recurrences of an LSTM handle launch per time step).
 * ec_lstm_step_fwd: a_in f32 [N,4H] = W_ih x + b_ih; whh [4H,H]; bhh [4H]; mask [N]; state_prev with row pitch ld_prev floats:
 *   ld_prev >= 2H -- rows [h | c] (h of actor n at state_prev + n*ld_prev, c at + H); ld_prev == H -- two dense blocks [2,N,H]
 *   (h first).  h_out / c_out: rows of pitch ld_h / ld_c >= H, not overlapping state_prev.  gates f32 [N,4H] out (i, f, g, o after
 *   their activations) or NULL.  Rows past N are never written.  H % 32 == 0 (and H % 256 == 0 or H <= 608), else EC_ERR_SHAPE;
 *   ld_prev a multiple of 4 and a_in, whh, state_prev 16-byte aligned.
 * ec_lstm_step_bwd: ONE reverse step.  dhs [N,H] = dL/dh_t from the heads; gates [N,4H], c [N,H] = c_t, c_prev [N,H] = m_t*c_{t-1}
 *   as the forward left them; mask [N] = m_t; da f32 [N,4H] out (gradient wrt a_t, gate order i, f, g, o); carry_c [N,H] in/out:
 *   dL/dc_t from step t+1 in, m_t*dc*f out.
 *   whhT == NULL (gate kernel + ec_gemm_f32, split-K 1): dh = dhs + carry_h; carry_h [N,H] in/out becomes m_t*(da whh).
 *   whhT != NULL (the fused step; H % 256 == 0, else EC_ERR_SHAPE): whhT f32 [H,4H] = whh transposed; dh = dhs +
 *     mask_next * (da_next whh) with da_next [N,4H], mask_next [N] of step t+1; carry_h and whh are not used (may be NULL).
 *   No float atomics on either route. */
int ec_lstm_step_fwd(const float* a_in, const float* whh, const float* bhh, const float* state_prev, long ld_prev,
                     const float* mask, float* h_out, long ld_h, float* c_out, long ld_c, float* gates, int N, int H,
                     ec_stream_t stream);
int ec_lstm_step_bwd(const float* dhs, const float* gates, const float* c, const float* c_prev, const float* mask,
                     const float* whh, const float* whhT, const float* da_next, const float* mask_next, float* carry_h,
                     float* carry_c, float* da, int N, int H, ec_stream_t stream);

/* One act step of an UPPER layer alone (rnn_stack.hip; what the act step of a multi-layer handle launches per layer l >= 1): the
 * input projection, the recurrent projection and the cell in one launch.  rnn_type EC_RNN_GRU | EC_RNN_LSTM; G = 3H | 4H.
 *   x f32, rows of pitch ld_x >= H floats: the layer's input (the state of the layer below);  wih, whh f32 [G,H];  bih, bhh [G];
 *   state_prev, rows of pitch ld_prev: h of actor n at state_prev + n*ld_prev (GRU: ld_prev >= H), and on an LSTM c at + H
 *   (ld_prev >= 2H);  mask f32 [N] multiplies the previous state, never x.
 *   h_out (pitch ld_h >= H), c_out (pitch ld_c >= H; LSTM only, ignored on a GRU), h_out2 (pitch ld_h2 >= H) or NULL: a second
 *   copy of h.  Rows past N are never written.
 * Alignment: x, wih, whh, state_prev 16-byte aligned and ld_x, ld_prev multiples of 4 floats (EC_ERR_ARG / EC_ERR_SHAPE).
 * Non-overlap: no output element may be an element of x or of the previous state of ANY actor (other workgroups still read
 *   those rows); slices of one state row at different column offsets do not overlap.
 * H % 32 == 0 and (H % 256 == 0 or H <= 608), else EC_ERR_SHAPE.  Wave partials are summed in a fixed order, the x part before
 * the h part: equal bits at every pitch and every actor slicing.  No atomics. */
int ec_rnn_stack_step_fwd(int rnn_type, const float* x, long ld_x, const float* wih, const float* whh, const float* bih,
                          const float* bhh, const float* state_prev, long ld_prev, const float* mask, float* h_out, long ld_h,
                          float* c_out, long ld_c, float* h_out2, long ld_h2, int N, int H, ec_stream_t stream);

/* ------------------------------------------------------------------------
 * Rollout post-processing and the PPO update ([U] allenact onpolicy_sync:
 * storage.py RolloutStorage.compute_returns, losses/ppo.py PPO.loss,
 * distributions.py CategoricalDistr, engine.py backprop_step).
 * ---------------------------------------------------------------------- */
/* rewards [T,N]; values, masks [T+1,N]; returns [T+1,N]; adv [T,N]; norm_adv [T,N] or NULL
 * ((adv-mean)/(unbiased std + eps) over the T*N local steps); stats2: 2 doubles scratch. */
int ec_gae(const float* rewards, const float* values, const float* masks, float* returns, float* adv,
           float* norm_adv, double* stats2, int T, int N, float gamma, float tau, float eps, ec_stream_t stream);
/* hv [B,A+1]; actions int64 [B]; old_logp, old_values, returns, norm_adv f32 [B];
 * dhv [B,A+1] out = grad_scale * d(total)/d(hv); sums4 out (doubles): sum over B of
 * {action loss, value loss, -entropy, ratio}; total = (s0 + vcoef*s1 + ecoef*s2)/B. */
int ec_ppo_loss(const float* hv, const int64_t* actions, const float* old_logp, const float* old_values,
                const float* returns, const float* norm_adv, float* dhv, double* sums4, long B, int A,
                float clip, float vcoef, float ecoef, float grad_scale, ec_stream_t stream);
/* As ec_ppo_loss with the value clip given separately: value_clip >= 0 is PPO(use_clipped_value_loss=True) with
 * that clip (AllenAct uses the same, possibly decayed, clip_param for both); value_clip < 0 is
 * use_clipped_value_loss=False, value loss = 0.5 (returns - values)^2.  An action id outside [0, A) makes
 * sums4[0] NaN (the loss fails loudly instead of scoring log-prob 0). */
int ec_ppo_loss_ex(const float* hv, const int64_t* actions, const float* old_logp, const float* old_values,
                   const float* returns, const float* norm_adv, float* dhv, double* sums4, long B, int A,
                   float clip, float value_clip, float vcoef, float ecoef, float grad_scale, ec_stream_t stream);
/* actions ~ Categorical(logits = hv[:, :A]); logp = log_prob(actions); values = hv[:, A] (or NULL).
 * The counter-based uniform of row n is keyed by (seed, step, first_actor + n), so a batch may be sampled in
 * slices (e.g. one per HIP stream) with identical results. */
int ec_sample_actions(const float* hv, int64_t* actions, float* logp, float* values, int N, int A,
                      uint64_t seed, uint64_t step, int first_actor, ec_stream_t stream);
/* actions = [U] CategoricalDistr.mode() of Categorical(logits = hv[:, :A]) -- the first index of the maximal logit;
 * logp = log_prob(actions); values = hv[:, A] (or NULL).  The deterministic action selection of an evaluation run (the
 * reference's `--eval` / `--run-type eval`: readme_files/baselines_robothor_objectnav.md:66-68, baselines_habitat.md:89-97,
 * zeroshot_objectnav.md:20-27); the stand-alone half of the two-call act step (any A). */
int ec_mode_actions(const float* hv, int64_t* actions, float* logp, float* values, int N, int A, ec_stream_t stream);
/* Episode bookkeeping of a rollout on the device: what [U] allenact's tasks and ScalarMeanTracker keep on the host and log
 * as `reward`, `ep_length`, `success` (restated; the metrics an evaluation run reports: readme_files/
 * baselines_robothor_objectnav.md:66-68, baselines_habitat.md:89-97, zeroshot_objectnav.md:20-27).  Conventions of ec_gae.
 * rewards f32 [T,N]; masks f32 [T+1,N] (masks[0] is not read); success f32 [T,N] or NULL (read at terminal steps only, NULL = 0).
 * For t = 0..T-1: carry_ret[n] += rewards[t,n] (fp32, step order), carry_len[n] += 1; masks[t+1,n] == 0 completes the
 * episode: it is added to totals5 (doubles: episodes, sum return, sum return^2, sum length, sum success), recorded, and both
 * carries restart at 0.  A running episode stays in the carries (f32 / int32 [N], in/out) for the next call.
 * Records (rec_f f32 [cap,2] = return, success; rec_i int32 [cap,3] = actor, t, length; both or neither may be NULL) are
 * appended at *n_records in a fixed order -- actor ascending, then t -- and dropped past cap, while *n_records (device
 * int32, in/out) and totals5 still count them: *n_records > cap tells the caller.  One workgroup, no floating-point
 * atomics: two runs give the same bits. */
int ec_episode_stats(const float* rewards, const float* masks, const float* success, float* carry_ret, int32_t* carry_len,
                     double* totals5, float* rec_f, int32_t* rec_i, int cap, int32_t* n_records, int T, int N,
                     ec_stream_t stream);
/* Navigation metrics of a rollout on the device: ec_episode_stats plus the path-efficiency scores the reference's result
 * tables give beside the success rate (SPL on RoboTHOR ObjectNav; SPL, SoftSPL and the distance to the goal on Habitat;
 * success and SPL per object type on readme_files/zeroshot_objectnav.md:20-48).  Restates [U] allenact's `spl_metric`
 * (RoboTHOR ObjectNav task) and [U] habitat-lab's `SPL` / `SoftSPL` measures from their published descriptions; neither
 * source is pinned.  Conventions of ec_episode_stats (masks [T+1,N], carries in/out, record order, records past cap).
 * step_dist f32 [T,N]: metres moved by step t, summed per episode in fp32, step order, in carry_path f32 [N] (in/out).
 * Read at the step that ends an episode only: start_dist f32 [T,N] (shortest-path length d0; < 0: no path), goal_dist f32
 * [T,N] or NULL (distance to the goal d1), category int64 with row stride N, rows 0..T-1 (or NULL; then C must be 0).
 * With p the path sum including step t and s the success flag, all in fp32:
 *   d0 <  0: spl = soft_spl = 0, the episode counts in no_path;
 *   d0 == 0: spl = soft_spl = (s > 0 && p == 0) ? 1 : 0;
 *   d0 >  0: ratio = d0 / max(d0, p); spl = s > 0 ? ratio : 0; soft_spl = max(0, 1 - d1 / d0) * ratio.
 * goal_dist NULL: soft_spl and the goal distance are not accumulated; their record fields are 0.
 * totals: double [(1 + C), 10], in/out -- row 0 all episodes, row 1 + c those of category c (an id outside [0, C) counts in
 * row 0 only); columns episodes, sum return, sum return^2, sum length, sum success, sum spl, sum soft_spl, sum goal_dist,
 * sum path, no_path.  0 <= C <= 64.
 * rec_f f32 [cap,7] = return, success, spl, soft_spl, path, goal_dist, start_dist; rec_i int32 [cap,4] = actor, t, length,
 * category (-1 without categories; an id outside [0, C) as given).  One workgroup, one launch, no floating-point atomics:
 * two runs give the same bits. */
int ec_nav_episode_stats(const float* rewards, const float* masks, const float* success, const float* step_dist,
                         const float* start_dist, const float* goal_dist, const int64_t* category, int C, float* carry_ret,
                         int32_t* carry_len, float* carry_path, double* totals, float* rec_f, int32_t* rec_i, int cap,
                         int32_t* n_records, int T, int N, ec_stream_t stream);
/* clip_grad_norm_(max_grad_norm) (<=0 disables) then Adam (1-based `step`) over n floats;
 * sumsq1: device scratch of ec_clip_adam_scratch_doubles() doubles; sumsq1[0] receives ||grads||^2 (the blocks' partial sums
 * and a ticket counter live behind it: the norm is folded in a fixed order, bit-identical run to run). */
int ec_clip_adam_scratch_doubles(void);
int ec_clip_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, double* sumsq1,
                      long n, float max_grad_norm, float lr, float beta1, float beta2, float eps, int step,
                      ec_stream_t stream);

/* ------------------------------------------------------------------------
 * Imitation learning ([U] allenact onpolicy_sync/losses/imitation.py Imitation.loss, the `expert_action` branch for a
 * CategoricalDistr; base_abstractions/distributions.py TeacherForcingDistr).  The training method of the reference's
 * rearrangement baselines (readme_files/baselines_ithor_rearrangement.md: DAgger) and of AllenAct's behaviour-cloning /
 * DAgger configurations of the ObjectNav and PointNav agents.  Restated from the published source; parity unpinned.
 * ---------------------------------------------------------------------- */
/* Expert cross-entropy, forward + analytic backward (restates Imitation.loss: -(mask * log_prob(expert)).sum() /
 * mask.sum().clamp(min=1)).  hv [B,A+1] (logits, value); expert_actions int64 [B]; expert_mask f32 [B]; 1 <= A <= 256.
 *   loss = -sum_b mask[b] * log_softmax(hv[b,:A])[e_b] / max(D, 1),  D = *denom (device memory) or, with denom NULL, this
 *   call's own sum of the mask (every block sums the whole mask in one order: no grid-wide synchronisation).
 *   sums3 (doubles, out) = {sum mask * (-logp_e), sum mask, sum mask * [first maximal logit of the row == e_b]} over this
 *   call's rows; the caller divides.
 *   dhv[b,k] = grad_scale * weight * mask[b] * (softmax_k - [k == e_b]) / max(D, 1).
 * accumulate == 0: dhv is written -- rows with mask 0 and the value column as zeros.  accumulate != 0: the term is ADDED to
 * dhv; rows with mask 0 and the value column are left alone ("PPO + imitation": ec_ppo_loss_ex first, then this call).
 * A row with mask 0 never reads its expert id; a row with mask != 0 and an id outside [0, A) makes sums3[0] NaN
 * (ec_ppo_loss_ex's rule).  A <= 16: one thread per row; above: one 64-lane wave per row.  Contiguous row chunks over several
 * workgroups; the blocks' partial sums go to scratch (ec_imitation_scratch_doubles() doubles, owned by one stream at a
 * time) and are folded in block order by the block that draws the last integer ticket -- no floating-point atomics: two
 * runs give the same bits, and with a shared denom a row's dhv does not depend on how the rows are split over calls.
 * Checked before any HIP call: NULL (but denom) -> EC_ERR_ARG; B <= 0 or A outside [1, 256] -> EC_ERR_SHAPE. */
int ec_imitation_scratch_doubles(void);
int ec_imitation_loss(const float* hv, const int64_t* expert_actions, const float* expert_mask, const double* denom,
                      float* dhv, double* sums3, double* scratch, long B, int A, float weight, float grad_scale,
                      int accumulate, ec_stream_t stream);
/* out[0] = sum over t < T, n0 <= n < n1 of expert_mask[t,n] (f32 [T,N]) in a fixed order: the normaliser mask.sum() of
 * Imitation.loss for the minibatch of samplers [n0, n1), computed once per rollout and shared by the calls that split it. */
int ec_expert_count(const float* expert_mask, int T, int N, int n0, int n1, double* out, ec_stream_t stream);
/* Teacher forcing after an act step (restates TeacherForcingDistr.sample / log_prob): actor n draws a uniform keyed by
 * (seed, step, first_actor + n) -- ec_sample_actions' key on a stream constant of its own, so it is not the sampler's draw --
 * and where expert_mask[n] != 0 and u < p: actions[n] = expert_actions[n], logp[n] = log_softmax(hv[n,:A])[expert].  Every
 * other row keeps what the act step wrote.  Slice-invariant like ec_sample_actions.  p outside [0, 1] -> EC_ERR_ARG; p == 0
 * launches nothing.  A forced id outside [0, A) gives logp NaN. */
int ec_teacher_force(const float* hv, const int64_t* expert_actions, const float* expert_mask, float p, int64_t* actions,
                     float* logp, int N, int A, uint64_t seed, uint64_t step, int first_actor, ec_stream_t stream);

/* ------------------------------------------------------------------------
 * Wide action spaces: up to 256 actions, ec_imitation_loss's bound (the reference's rearrangement experiment has 84:
 * readme_files/baselines_ithor_rearrangement.md).  The narrow entry points keep their limits -- ec_policy_act* 7 actions,
 * ec_ppo_loss_ex 16 -- and their kernels; these run kernels of their own (csrc/wide_actions.hip).
 * ---------------------------------------------------------------------- */
/* The actor and critic heads with the action selection in the same launch:
 *   hv[b,:A] = hs[b] . Wa^T + ba,  hv[b,A] = hs[b] . wc + bc      hs f32 [B,H], Wa [A,H], ba [A], wc [H], bc [1], hv [B,A+1].
 * 1 <= A <= 256, H % 4 == 0 (and H <= 3576: a workgroup keeps its four rows of hs in LDS, above is EC_ERR_UNSUPPORTED).
 * actions NULL: logits and values only.  Otherwise, once a row's A + 1 outputs exist, the same launch selects:
 *   greedy == 0: ec_sample_actions' draw, keyed by (seed, step, first_actor + b);   greedy != 0: ec_mode_actions' first
 *   maximal logit;   logp = log_prob(action), values = hv[:,A] (or NULL).
 *   expert_actions / expert_mask / force_p (NULL, NULL, 0 = none; sampling only): ec_teacher_force's rule and uniform -- a row
 *   with mask 0 never reads its expert id, a forced id outside [0, A) gives that action with logp NaN.
 * actions / logp / values are bit-identical to ec_sample_actions / ec_mode_actions (then ec_teacher_force) run on the hv this
 * launch wrote: the exp terms are computed across lanes, the sums of the log-sum-exp and of the CDF in their index order.
 * A row's outputs do not depend on B or on the rows that share its workgroup.
 * Checked before any HIP call: NULL, forcing with greedy or without actions, force_p outside [0, 1] or without expert
 * arrays -> EC_ERR_ARG; B <= 0, A outside [1, 256], H % 4 -> EC_ERR_SHAPE. */
int ec_heads_wide(const float* hs, const float* Wa, const float* ba, const float* wc, const float* bc, float* hv, long B, int H,
                  int A, int64_t* actions, float* logp, float* values, int greedy, uint64_t seed, uint64_t step,
                  int first_actor, const int64_t* expert_actions, const float* expert_mask, float force_p, ec_stream_t stream);
/* The act step in one call for every handle: 1 <= num_actions <= 256, integer or coordinate goals (exactly one of goal /
 * goal_vec, by the handle's type), dual, fusion.  Arguments of ec_policy_act plus goal_vec, greedy and the forcing triple of
 * ec_heads_wide (forcing with greedy -> EC_ERR_ARG).
 *   more than 7 actions: ec_policy_forward2's stages up to the recurrence (T = 1, EC_POLICY_INFER[_REUSE]; the same
 *     workspace), then ec_heads_wide's launch on actor.linear.* / critic.fc.* where they lie in `params`;
 *   up to 7 actions: exactly the launches of ec_policy_act / _vec / _greedy, then ec_teacher_force's when forcing is asked. */
int ec_policy_act_ex(const ec_policy_t* h, const float* params, const void* feat, const void* feat2, int feat_bf16,
                     const int64_t* goal, const float* goal_vec, const float* h0, const float* masks, int N, void* workspace,
                     size_t ws_bytes, int reuse_tables, float* hv, float* h_final, int64_t* actions, float* logp, float* values,
                     int greedy, uint64_t seed, uint64_t step, int first_actor, const int64_t* expert_actions,
                     const float* expert_mask, float force_p, ec_stream_t stream);
/* ec_ppo_loss_ex for 1 <= A <= 256: the same per-row arithmetic with one 64-lane wave per row (lane-strided logits, xor
 * butterflies for the maximum and the sums) and contiguous row chunks over several workgroups.  The blocks' fp64 partials of
 * the four sums go to scratch (ec_ppo_loss_wide_scratch_doubles() doubles, owned by one stream at a time) and are folded in
 * block order by the block that draws the last integer ticket: two runs give the same bits, and a row's dhv depends on the
 * row and on grad_scale / B alone. */
int ec_ppo_loss_wide_scratch_doubles(void);
int ec_ppo_loss_wide(const float* hv, const int64_t* actions, const float* old_logp, const float* old_values,
                     const float* returns, const float* norm_adv, float* dhv, double* sums4, double* scratch, long B, int A,
                     float clip, float value_clip, float vcoef, float ecoef, float grad_scale, ec_stream_t stream);

/* ------------------------------------------------------------------------
 * Previous-action embedding of the recurrent input ([U] habitat_baselines PointNavResNetPolicy: prev_action_embedding =
 * nn.Embedding(num_actions + 1, 32) indexed by ((prev_actions.float() + 1) * masks).long(); [U] allenact VisualNavActorCritic:
 * add_prev_actions / action_embed_size / add_prev_action_null_token).  Restated from the published sources, which are not
 * under the reference tree: parity unpinned.  The kernels alone first, then the policy entry points that use them.
 *   A = number of actions (1..256), null_token in {0, 1}, R = A + null_token table rows, E = embedding width (1..64),
 *   G = 3 * hidden gate columns, B = T * N frames; emb [R, E]; Wa = columns col0 .. col0 + E of a row-major matrix w with G
 *   rows and leading dimension ld >= col0 + E (any ld: nothing here needs ld to be a multiple of 4).
 *   idx[b] = null_token ? (masks[b] != 0 ? prev_actions[b] + 1 : 0) : prev_actions[b]
 * An index outside [0, R) is never dereferenced: that frame adds nothing to gi and contributes nothing to any gradient.
 * masks may be NULL when null_token is 0.  No floating-point atomics: two runs give the same bits. */
/* pt[r, g] = sum_e emb[r, e] * w[g * ld + col0 + e], fp32 FMA in ascending e; pt [R, G] */
int ec_prev_action_table(const float* emb, const float* w, long ld, int col0, float* pt, int A, int null_token, int G, int E,
                         ec_stream_t stream);
/* gi[b, :] += pt[idx[b], :]; gi [B, G] dense */
int ec_prev_action_add(float* gi, const float* pt, const int64_t* prev_actions, const float* masks, int null_token, int A, long B,
                       int G, ec_stream_t stream);
/* dPT[r, :] = sum over {b : idx[b] == r} of dgi[b, :], then demb[r, e] += sum_g dPT[r, g] * Wa[g, e] (four contiguous quarters of
 * g, each in ascending order, folded in order) and dw[g * ld + col0 + e] += sum_r dPT[r, g] * emb[r, e] (ascending r): both ADD
 * onto what is there.
 * The frames are cut into P = ceil(B / chunk) partitions of chunk = max(R, 128, ceil(B / 4096)) consecutive frames -- a function
 * of B and R alone; a partition is summed in ascending b per (row, column), the partitions are folded in ascending order.  A
 * table row that no frame selects has dPT == 0 exactly and adds exactly 0.
 * scratch: ec_prev_action_grad_scratch_floats(B, G, A, null_token) = (P + 1) * R * G floats, owned by one stream at a time;
 * since chunk >= R, P * R < B + R: the partitions' bins take less than (B + R) * G floats -- 1 / 18 of dgi for B = 32768, R = 7 --
 * and on return scratch[0 .. R * G) holds dPT. */
size_t ec_prev_action_grad_scratch_floats(long B, int G, int A, int null_token);
int ec_prev_action_grad(const float* dgi, const int64_t* prev_actions, const float* masks, int null_token, int A, const float* emb,
                        const float* w, long ld, int col0, float* demb, float* dw, float* scratch, long B, int G, int E,
                        ec_stream_t stream);
/* prev_action_dims > 0 handles.  ec_policy_forward_pa: the arguments of ec_policy_forward_vec with BOTH goal arguments (exactly
 * one non-NULL, by the handle's goal type) and prev_actions int64 [T*N], row t * N + n = the action actor n took at step t - 1.
 * ec_policy_act_pa: the arguments of ec_policy_act_ex and prev_actions int64 [N]: sampling, greedy selection, forcing, narrow
 * and wide heads, both goal types.  Where the table is added: inside gi_act_kernel's fold, next to the bias, on the act step's
 * 1568-wide route (an EC_POLICY_INFER_REUSE act step then issues exactly the launches of a prev_action_dims == 0 handle);
 * ec_prev_action_add's launch behind the input projection on every other route (onto part 0 of a split-K projection).  A learn
 * pass leaves the indices in its workspace; ec_policy_backward* then adds the embedding's gradient and columns flat.. of
 * weight_ih's with ec_prev_action_grad's launches before `recurrent_grads_ready` is recorded.  An actor's result does not
 * depend on how the actors are sliced; ec_policy_act_pa equals ec_policy_forward_pa at T = 1 followed by ec_sample_actions /
 * ec_mode_actions bit for bit; with a zero embedding every output and every other tensor's gradient equals, bit for bit, those
 * of the prev_action_dims == 0 handle that holds weight_ih[:, :flat] (the launch plan does not depend on prev_action_dims).
 * Checked before any HIP call: every other forward / act entry point returns EC_ERR_ARG on such a handle; these return
 * EC_ERR_ARG on a prev_action_dims == 0 handle and for a NULL prev_actions. */
int ec_policy_forward_pa(const ec_policy_t* h, const float* params, const void* feat, const void* feat2, int feat_bf16,
                         const int64_t* goal, const float* goal_vec, const int64_t* prev_actions, const float* h0,
                         const float* masks, int T, int N, void* workspace, size_t ws_bytes, int for_backward, float* hv,
                         float* h_final, ec_stream_t stream);
int ec_policy_act_pa(const ec_policy_t* h, const float* params, const void* feat, const void* feat2, int feat_bf16,
                     const int64_t* goal, const float* goal_vec, const int64_t* prev_actions, const float* h0, const float* masks,
                     int N, void* workspace, size_t ws_bytes, int reuse_tables, float* hv, float* h_final, int64_t* actions,
                     float* logp, float* values, int greedy, uint64_t seed, uint64_t step, int first_actor,
                     const int64_t* expert_actions, const float* expert_mask, float force_p, ec_stream_t stream);

/* ------------------------------------------------------------------------
 * The pooled-embedding net: habitat-lab's PointNavResNetNet over ONE vector per frame (the pooled CLIP embedding) -- the
 * Habitat DD-PPO branch of readme_files/baselines_habitat.md.  [U] restated from the published habitat-lab sources
 * (habitat_baselines/rl/ddppo/policy/resnet_policy.py), which are not under the reference tree: parity unpinned.
 *   v   = ReLU(W_fc e + b_fc)                      e: pooled embedding [D]; visual_fc W_fc [H, D]
 *   x   = [ v | Emb_goal[goal] | W_1 s_1 + b_1 | ... | W_S s_S + b_S | Emb_prev[(prev + 1) * mask] ]
 *   h   = RNN(x, m * h_prev)                       GRU | LSTM, 1..EC_RNN_MAX_LAYERS layers
 *   logits = W_a h + b_a ; value = W_c h + b_c
 * s_i are small float sensors (PointNav's (rho, cos -phi, sin -phi); ObjectNav's GPS and (cos c, sin c) compass); the caller
 * hands over the embeddings' inputs, the polar / compass transforms are its own.
 * Flat parameter order: visual_fc weight [H, D], bias [H]; obj_categories_embedding.weight [num_goals, embed_dims] if
 * num_goals > 0; per sensor weight [embed_dims, k_i], bias [embed_dims]; state_encoder.rnn.{weight_ih,weight_hh,bias_ih,bias_hh}_l0
 * with weight_ih_l0 [G, H + embed_dims * (ids + S) + E] (ids = num_goals > 0; column order: the x above); actor weight, bias;
 * critic weight, bias; prev_action_embedding.weight [A + null, E] if E > 0; the upper layers' four tensors per layer.
 * Nothing [T*N, embed_dims]-shaped exists: every side input reaches the input projection through weight-derived tables
 * (Wg, W_i', Wp: the column blocks of weight_ih_l0 behind its first H columns)
 *   GT = Emb_goal Wg^T [num_goals, G];  PT = ec_prev_action_table;  SV[:, cols_i] = W_i' W_i [G, K];  sb = sum_i W_i' b_i [G]
 *   gi = v weight_ih_l0[:, :H]^T + b_ih + sb + GT[goal] + PT[row] + SV s     (s: the K = sum k_i sensor floats, k ascending)
 * built per EC_POLICY_INFER call, kept under EC_POLICY_INFER_REUSE, rebuilt per learn pass, with a dense [G, H] copy of
 * weight_ih_l0[:, :H]: no GEMM reads weight_ih_l0 in place.  No float atomics on any route of such a handle: two learn passes
 * give equal bits, and an actor's result does not depend on how the actors are sliced.
 * ec_policy_create_pooled: EC_ERR_ARG for a NULL argument, num_goals == 0 && num_sensors == 0 (the net needs a goal),
 * num_sensors outside 0..3, a sensor width < 1, K > 8, embed_dims outside 1..64, num_goals outside 0..256, num_actions outside
 * 2..256, the previous-action fields as in ec_policy_cfg, rnn_type / num_layers as in ec_policy_create_rnn_layers;
 * EC_ERR_SHAPE for embed_in outside 64..4096 or % 4, and for a hidden ec_policy_create_rnn(EC_RNN_LSTM) refuses.
 * The handle answers ec_policy_num_param_tensors / _flat_size / _param_offset / _workspace_bytes / _state_width / _rnn_type /
 * _rnn_layers / _destroy, and ec_policy_backward3 (feat = the embedding rows f32 [T*N, D]; feat2 and feat_bf16 are ignored).
 * Every other forward / act entry point returns EC_ERR_ARG on it, and the two below EC_ERR_ARG on every other handle.
 * ---------------------------------------------------------------------- */
typedef struct {
    int embed_in;        /* D: 64..4096, % 4 == 0 */
    int hidden;          /* H: the widths ec_policy_create_rnn admits */
    int embed_dims;      /* 32; 1..64: width of the goal-id embedding and of every sensor embedding */
    int num_goals;       /* 0: no goal-id embedding; else nn.Embedding(num_goals, embed_dims) */
    int num_sensors;     /* 0..3 */
    int sensor_in[3];    /* k_i >= 1, K = sum k_i <= 8 */
    int num_actions;     /* 2..256 */
    int prev_action_dims, prev_action_null;   /* as in ec_policy_cfg */
    int rnn_type, num_layers;                 /* EC_RNN_GRU | EC_RNN_LSTM, 1..EC_RNN_MAX_LAYERS */
} ec_pooled_cfg;
int ec_policy_create_pooled(ec_policy_t** out, const ec_pooled_cfg* cfg);
int ec_policy_is_pooled(const ec_policy_t* h);         /* 1 | 0 (0: NULL handle) */
/* embed f32 [T*N, D] (16-byte aligned); goal int64 [T*N] (num_goals > 0) | NULL; sensors f32 [T*N, K] (num_sensors > 0) | NULL;
 * prev_actions int64 [T*N] (prev_action_dims > 0) | NULL -- a NULL argument must match a part the handle does not have, and the
 * reverse, else EC_ERR_ARG.  The other arguments: ec_policy_forward2's.  A goal id outside [0, num_goals) adds nothing.  A learn
 * pass leaves goal ids, sensors and previous actions in the workspace for ec_policy_backward3.
 * T > 1, and T = 1 on the general route: ec_gemm_f32 with ReLU, an ec_gemm_f32 input projection, one rows-add launch for the
 * tables, then the step kernels and heads of every other handle.  T = 1 inference with D % 56 == 0 or D % 64 == 0 and
 * h_final != h0 (EC_POOLED_ACT=0 in the environment: the general route): 2 + L launches with reused tables --
 * pooled_fc_act_kernel, pooled_step0_kernel (layer 0: both projections, the table rows and the cell), one rnn_stack launch per
 * upper layer, the heads.  Inference heads: up to 7 actions the one-wave-per-row launch, above it ec_heads_wide's launch (with
 * or without a selection), so a row of hv does not depend on how the actors are sliced on any inference route. */
int ec_policy_forward_pooled(const ec_policy_t* h, const float* params, const float* embed, const int64_t* goal,
                             const float* sensors, const int64_t* prev_actions, const float* h0, const float* masks, int T, int N,
                             void* workspace, size_t ws_bytes, int for_backward, float* hv, float* h_final, ec_stream_t stream);
/* The same at T = 1 in one call with the selection arguments of ec_policy_act_ex (2..256 actions: the narrow sampling heads
 * up to 7, ec_heads_wide above): bit for bit ec_policy_forward_pooled followed by the stand-alone selection. */
int ec_policy_act_pooled(const ec_policy_t* h, const float* params, const float* embed, const int64_t* goal, const float* sensors,
                         const int64_t* prev_actions, const float* h0, const float* masks, int N, void* workspace,
                         size_t ws_bytes, int reuse_tables, float* hv, float* h_final, int64_t* actions, float* logp, float* values,
                         int greedy, uint64_t seed, uint64_t step, int first_actor, const int64_t* expert_actions,
                         const float* expert_mask, float force_p, ec_stream_t stream);
/* The two act-step kernels alone (tests, benchmarks).
 * ec_pooled_fc_act: v [N, H] = ReLU(e [N, D] w [H, D]^T + b); wfrag: H * D floats of scratch that receive w in MFMA fragment
 *   order.  A workgroup owns a 32 x 32 output tile, its 7 (D % 56 == 0) or 8 (D % 64 == 0) waves split K = D on
 *   v_mfma_f32_32x32x2_f32 and fold through LDS in wave order.  EC_ERR_SHAPE unless one of the two holds and H % 32 == 0;
 *   EC_ERR_ARG for a NULL or misaligned (16 bytes) e, w, wfrag.
 * ec_pooled_step0_fwd: ec_rnn_stack_step_fwd whose x half also receives, in this order, sb [G] | NULL, gt[goal[n]] ([num_goals, G],
 *   goal int64 [N]) | both NULL, pt[row(prev[n], mask[n])] ([A + null_token, G], prev int64 [N]) | both NULL, and
 *   sum_k sv[:, k] sensors[n, k] (sv [G, K], sensors [N, K], K <= 8, k ascending) | both NULL.  In place (h_out == state_prev)
 *   is refused with EC_ERR_ARG: a workgroup reads rows of state_prev that another one writes. */
int ec_pooled_fc_act(const float* e, const float* w, const float* b, float* wfrag, float* v, int N, int D, int H, ec_stream_t stream);
int ec_pooled_step0_fwd(int rnn_type, const float* x, long ld_x, const float* wih, const float* whh, const float* bih,
                        const float* bhh, const float* sb, const float* gt, const int64_t* goal, int num_goals, const float* pt,
                        const int64_t* prev_actions, int null_token, int A, const float* sv, const float* sensors, int K,
                        const float* state_prev, long ld_prev, const float* mask, float* h_out, long ld_h, float* c_out, long ld_c,
                        float* h_out2, long ld_h2, int N, int H, ec_stream_t stream);

/* ------------------------------------------------------------------------
 * The two-view rearrangement net: the 1-Phase Embodied CLIP ResNet50 IL agent of
 * readme_files/baselines_ithor_rearrangement.md.  [U] restated from the published ai2thor-rearrangement / allenact sources
 * (ResNetRearrangeActorCriticRNN), which are not under the reference tree: parity unpinned.  Per frame, u and w are the frozen
 * CLIP maps [S2, C] (NHWC rows, bf16) of the current view and of the goal-state view from the same pose, c_p = [u_p | w_p | u_p * w_p]:
 *   e_p = ReLU(W_e c_p + b_e)                      visual_encoder.0      Conv2d(3C, H, 1)
 *   m_p = ReLU(W_a c_p + b_a)                      visual_attention.0    Conv2d(3C, A1, 1), A1 = 32
 *   l_p = <w_2, m_p> + b_2                         visual_attention.2    Conv2d(A1, 1, 1)
 *   a   = softmax_p(l)                             over the S2 pixels of the frame
 *   v   = (1/S2) sum_p a_p e_p                     a MEAN over the pixels, not a sum
 *   x   = [ v | Emb_prev[(prev + 1) * mask] ]      then the recurrent core and the heads of the pooled-embedding net
 * Unlike every other front this one is TRAINABLE (the towers stay frozen: no gradient reaches u or w).
 * Flat parameter order: visual_encoder.0 weight [H, 3C], bias [H]; visual_attention.0 weight [A1, 3C], bias [A1];
 * visual_attention.2 weight [1, A1], bias [1]; state_encoder.rnn.{weight_ih,weight_hh,bias_ih,bias_hh}_l0 with weight_ih_l0
 * [G, H + E]; actor weight, bias; critic weight, bias; prev_action_embedder.weight [A + null, E] if E > 0; the upper layers' four
 * tensors per layer.
 * The plan is the pooled-embedding handle's from v onwards (dense copy of weight_ih_l0[:, :H], the previous-action table, step
 * kernels, rnn_stack for upper layers, wide / narrow heads); v is not rectified after pooling, so the backward masks nothing on
 * dv.  On THIS handle the previous-action width E may reach 512 (upstream's is H): above 64 the table PT = Emb W_ih[:, H:]^T and
 * its chain to the two gradients run on ec_gemm_f32 (K in one piece) behind the same binned ordered sum over frames.
 * No float atomics on any route: two learn passes give equal bits, an actor's result does not depend on how the actors are sliced.
 * ec_policy_create_two_view: EC_ERR_ARG for a NULL argument, num_actions outside 2..256, prev_action_dims outside 0..512,
 * prev_action_null not 0 | 1 or set without prev_action_dims, rnn_type / num_layers as in ec_policy_create_rnn_layers;
 * EC_ERR_SHAPE for in_channels outside 64..4096 or % 64, spatial * spatial outside 1..64, attn_hidden outside 32..128 or % 32, and
 * for a hidden ec_policy_create_rnn(EC_RNN_LSTM) refuses.
 * The handle answers ec_policy_num_param_tensors / _flat_size / _param_offset / _workspace_bytes / _state_width / _rnn_type /
 * _rnn_layers / _destroy, and ec_policy_backward3 (feat = u, feat2 = w, both bf16: feat_bf16 = 0 or a NULL feat2 is EC_ERR_ARG).
 * Every other forward / act entry point returns EC_ERR_ARG on it, and the two below EC_ERR_ARG on every other handle.
 * ---------------------------------------------------------------------- */
typedef struct {
    int in_channels;     /* C: 64..4096, % 64 == 0 */
    int spatial;         /* 7: S2 = spatial * spatial in 1..64 */
    int hidden;          /* H: the widths ec_policy_create_rnn(EC_RNN_LSTM) admits */
    int attn_hidden;     /* A1 = 32; 32..128, % 32 == 0 */
    int num_actions;     /* 2..256 */
    int prev_action_dims, prev_action_null;   /* E in 0..512; null as in ec_policy_cfg */
    int rnn_type, num_layers;                 /* EC_RNN_GRU | EC_RNN_LSTM, 1..EC_RNN_MAX_LAYERS */
} ec_two_view_cfg;
int ec_policy_create_two_view(ec_policy_t** out, const ec_two_view_cfg* cfg);
int ec_policy_is_two_view(const ec_policy_t* h);       /* 1 | 0 (0: NULL handle) */
/* feat = u, feat2 = w: bf16 [T*N, S2, C], 16-byte aligned; prev_actions int64 [T*N] (prev_action_dims > 0) | NULL -- NULL must
 * match a handle without the embedding, and the reverse, else EC_ERR_ARG.  The other arguments: ec_policy_forward2's.  A learn
 * pass leaves the attention probabilities, the post-ReLU activations of both convs and the previous actions in the workspace
 * for ec_policy_backward3.  T = 1 inference with h_final != h0 (EC_POOLED_ACT=0: the general route): the front's launch, then
 * pooled_step0_kernel, one rnn_stack launch per upper layer and the heads, as on the pooled-embedding handle. */
int ec_policy_forward_two_view(const ec_policy_t* h, const float* params, const void* feat, const void* feat2,
                               const int64_t* prev_actions, const float* h0, const float* masks, int T, int N, void* workspace,
                               size_t ws_bytes, int for_backward, float* hv, float* h_final, ec_stream_t stream);
/* The same at T = 1 in one call with the selection arguments of ec_policy_act_pooled: bit for bit
 * ec_policy_forward_two_view followed by the stand-alone selection. */
int ec_policy_act_two_view(const ec_policy_t* h, const float* params, const void* feat, const void* feat2,
                           const int64_t* prev_actions, const float* h0, const float* masks, int N, void* workspace,
                           size_t ws_bytes, int reuse_tables, float* hv, float* h_final, int64_t* actions, float* logp, float* values,
                           int greedy, uint64_t seed, uint64_t step, int first_actor, const int64_t* expert_actions,
                           const float* expert_mask, float force_p, ec_stream_t stream);
/* The front's two kernels alone (tests, benchmarks; two_view.hip).  u, w bf16 [B, S2, C]; We [H, 3C], be [H], Wa [A1, 3C],
 * ba [A1], w2 [A1], b2 [1]; v f32 [B, H].  Shapes: C % 64 == 0 in 64..4096, S2 in 1..64, H as above, A1 % 32 == 0 in 32..128,
 * else EC_ERR_SHAPE; NULL or a misaligned (16 bytes) u, w, We, Wa, dWe, dWa, workspace -> EC_ERR_ARG; a short workspace ->
 * EC_ERR_WORKSPACE.  ec_two_view_workspace_bytes: 0 for a refused shape.
 * ec_two_view_fwd: K = 3C walked once on v_mfma_f32_32x32x16_bf16 against the combined [A1 + H, 3C] weight as three bf16 planes;
 *   the product columns are formed while staging (exact: two bf16 planes), [u | w | u * w] never exists in memory.  A workgroup
 *   owns whole frames (3 frames of 49 pixels in 160 rows: 91.9 % useful rows; 1 in 64 for launches of few frames); a frame's v
 *   has the same bits however the frames are sliced.  save != 0 (workspace sized with for_backward = 1): keeps the probabilities
 *   and both convs' post-ReLU activations for ec_two_view_bwd.
 * ec_two_view_bwd: ADDS the six gradients of sum(v * dv) onto dWe, dbe, dWa, dba, dw2, db2, from the workspace the saving
 *   forward of the same shapes left.  Ordered sums only: two calls give equal bits. */
size_t ec_two_view_workspace_bytes(long B, int S2, int C, int H, int A1, int for_backward);
int ec_two_view_fwd(const void* u, const void* w, const float* We, const float* be, const float* Wa, const float* ba,
                    const float* w2, const float* b2, float* v, long B, int S2, int C, int H, int A1, void* workspace,
                    size_t ws_bytes, int save, ec_stream_t stream);
int ec_two_view_bwd(const void* u, const void* w, const float* w2, const float* dv, float* dWe, float* dbe, float* dWa,
                    float* dba, float* dw2, float* db2, long B, int S2, int C, int H, int A1, void* workspace, size_t ws_bytes,
                    ec_stream_t stream);

/* ------------------------------------------------------------------------
 * CLIP VisionTransformer embedder == [U] allenact ClipViTEmbedder.forward over
 * [U] openai/CLIP VisionTransformer: patch-embed, class +
 * positional embedding, ln_pre, then `layers_run` ResidualAttentionBlocks
 * (ClipViTPreprocessor runs all but the LAST block; no ln_post / proj).
 * w_bf16 (concatenated): conv1 as [D][P*P*3] with K ordered (ky,kx,c); then per block
 *   in_proj_weight [3D,D], out_proj.weight [D,D], mlp.c_fc.weight [4D,D], mlp.c_proj.weight [D,4D].
 * params_f32: class_embedding [D], positional_embedding [L,D], ln_pre.{w,b}; then per block
 *   ln_1.{w,b}, in_proj_bias [3D], out_proj.bias [D], ln_2.{w,b}, c_fc.bias [4D], c_proj.bias [D].
 * ---------------------------------------------------------------------- */
typedef struct ec_vit ec_vit_t;
int ec_vit_create(ec_vit_t** out, int width, int layers_run, int heads, int patch, int input_resolution,
                  const void* w_bf16, size_t n_w, const float* params_f32, size_t n_f);
void ec_vit_destroy(ec_vit_t* h);
int ec_vit_tokens(const ec_vit_t* h);                       /* L = (R/P)^2 + 1 */
int ec_vit_set_conv8_min_tiles(ec_vit_t* h, int n);          /* as ec_rn50_set_conv8_min_tiles */
uint64_t ec_vit_plan_hash(const ec_vit_t* h);                /* as ec_rn50_plan_hash */
size_t ec_vit_workspace_bytes(const ec_vit_t* h, int batch);
/* rgb f32 NHWC [B,R,R,3] -> tokens bf16 [B, L, D] */
int ec_vit_forward(const ec_vit_t* h, const float* rgb_nhwc, int batch, void* workspace, size_t ws_bytes,
                   void* tokens_bf16, ec_stream_t stream);
/* out[r, c] = (float) in[r*in_stride + c]  -- the `.float()` at the API edge (e.g. class_emb_only: in_stride = L*D) */
int ec_bf16_to_f32(const void* in, float* out, long rows, long row_len, long in_stride, ec_stream_t stream);

/* ------------------------------------------------------------------------
 * The class embedding alone ([U] allenact ClipViTEmbedder with class_emb_only: `x[:, 0, :]` after resblocks[:-1]):
 * rgb f32 NHWC [B,R,R,3] -> out f32 [B, D], bf16 values (what ec_vit_forward + ec_bf16_to_f32 on row 0 deliver).
 * Two routes: the general one (ec_vit_forward into the workspace, then row 0), and the CLS tail -- the last block that
 * runs computes K / V for all tokens but q, the attention row, out_proj, ln_2 and the MLP for the B class rows only
 * (vit_cls.hip).  EC_VIT_CLS_TAIL = 0 / 1 forces the general route / the tail; unset, the library's rule picks per
 * (tokens, frames).  The two routes round at the same points but are not bit-identical.
 *
 * Stage entry points of the tail's kernels (arguments checked before any HIP call: NULL or a misaligned pointer ->
 * EC_ERR_ARG, a bad shape or pitch -> EC_ERR_SHAPE):
 *   ec_gemm_rows_bf16: out[M, N] = act(A[M, K] W[N, K]^T + bias (+ res)) for few rows: a workgroup owns 32 columns of up
 *     to 128 rows and its four waves split K.  A bf16 at row pitch lda, W bf16 [N, K], bias f32 [N] or NULL, res bf16 at
 *     row pitch ldr or NULL, out at row pitch ldo (pitches in elements).  act: EC_ACT_NONE | EC_ACT_QUICKGELU.
 *     store: 0 bf16, 1 rounded to bf16 and written as f32, 2 f32.  K % 64 == 0, N % 32 == 0, lda % 8 == 0.
 *   ec_vit_cls_rows_ln: nn.LayerNorm(D), eps 1e-5, of `rows` bf16 rows read at pitch `pitch` (elements) -> bf16 [rows, D].
 *   ec_vit_cls_attn: one query per (frame, head): q bf16 [B, D], kv bf16 [B*L, 2D] (k | v) -> out bf16 [B, D];
 *     softmax(q k^T / 8) v, D / heads == 64, 1 <= L <= 512.
 * ---------------------------------------------------------------------- */
size_t ec_vit_cls_workspace_bytes(const ec_vit_t* h, int batch);
int ec_vit_embed_cls(const ec_vit_t* h, const float* rgb_nhwc, int batch, void* workspace, size_t ws_bytes, float* out,
                     ec_stream_t stream);
int ec_gemm_rows_bf16(const void* A, long lda, const void* W, const float* bias, const void* res, long ldr, void* out, long ldo,
                      int M, int N, int K, int act, int store, ec_stream_t stream);
int ec_vit_cls_rows_ln(const void* x, long pitch, const float* gamma, const float* beta, void* out, int rows, int D,
                       ec_stream_t stream);
int ec_vit_cls_attn(const void* q, const void* kv, void* out, int B, int L, int D, int heads, ec_stream_t stream);

/* ------------------------------------------------------------------------
 * [U] openai/CLIP AttentionPool2d.forward, the module the reference detaches and calls on the conv
 * features (primitive_probing/generate_data/thor_image_features.py:62,112): mean token + positional
 * embedding, q/k/v projections, 64-wide heads, softmax, c_proj; returns token 0 only, so only the
 * CLS query is computed.  feat bf16 NHWC [B,HW,C]; wkv = [k_proj.weight; v_proj.weight] ([2C,C]),
 * bkv likewise; out f32 [B,out_dim].
 * ---------------------------------------------------------------------- */
size_t ec_attnpool_workspace_bytes(int batch, int HW, int C);
int ec_attnpool_forward(const void* feat, int batch, int HW, int C, int heads, int out_dim, const float* pos,
                        const void* wq, const float* bq, const void* wkv, const float* bkv, const void* wc,
                        const float* bc, void* workspace, size_t ws_bytes, float* out, ec_stream_t stream);

/* ------------------------------------------------------------------------
 * CLIP text tower == CLIP.encode_text ([U] openai/CLIP clip/model.py; the goal embedding of the zero-shot
 * ObjectNav variant, readme_files/zeroshot_objectnav.md:3-8): token + positional embedding, `layers` causal
 * ResidualAttentionBlocks, ln_final, features at the EOT token (arg-max id) @ text_projection.
 * w_bf16: per block in_proj [3D][D], out_proj [D][D], c_fc [4D][D], c_proj [D][4D]; then text_projection^T [E][D].
 * params_f32: token_embedding [vocab][D], positional_embedding [ctx][D], per block ln_1 w,b, in_proj_bias [3D],
 * out_proj.bias, ln_2 w,b, c_fc.bias [4D], c_proj.bias; then ln_final w,b.  tokens int32 [B][ctx] (the BPE tokenizer
 * is host string processing, not part of this path); out f32 [B][E].  width/heads must be 64, ctx <= 512.
 * ---------------------------------------------------------------------- */
typedef struct ec_text ec_text_t;
int ec_text_create(ec_text_t** out, int width, int layers, int heads, int context_length, int vocab_size,
                   int embed_dim, const void* w_bf16, size_t n_w, const float* params_f32, size_t n_f);
void ec_text_destroy(ec_text_t* h);
size_t ec_text_workspace_bytes(const ec_text_t* h, int batch);
int ec_text_forward(const ec_text_t* h, const int32_t* tokens, int batch, void* workspace, size_t ws_bytes,
                    float* out, ec_stream_t stream);

/* ------------------------------------------------------------------------
 * Linear probe heads (BASELINE config 1) == LinearEncoder of
 * primitive_probing/train.py:14-113.  The Linear / Conv1x1 contraction is ec_gemm_f32; these are the
 * activation + loss + metric counts + analytic backward of compute_loss (train.py:56-92):
 *   EC_PROBE_SIGMOID_BCE         Sigmoid + F.binary_cross_entropy over [R,C]  (object_presence; object_localization
 *                                with R = B*9 rows from ec_probe_pool3)                     train.py:29,31,44-49,76
 *   EC_PROBE_SIGMOID_BCE_GATHER  Sigmoid, loss on column idx[r] only (reachability)         train.py:61-63,72,76
 *   EC_PROBE_SOFTMAX_CE2         Softmax(dim=1) then F.cross_entropy ON THE PROBABILITIES   train.py:35,78
 *                                (double softmax reproduced); labels > label_clamp are clamped (train.py:65)
 * labels int64: [R,C] (mode 0) or [R] (modes 1,2); idx int64 [R] (mode 1).
 * pred [R,C] (probabilities), dlogits [R,C] = d(mean loss)/d(logits), dbias [C] = column sums of dlogits:
 * each may be NULL.  out5 (doubles): {sum of per-element losses, tp, pred_pos, true_pos, correct}; the mean
 * loss is out5[0] / (R*C) (mode 0) or / R (modes 1,2); micro-F1 = 2 tp / (pred_pos + true_pos) (train.py:86),
 * accuracy = correct / count (train.py:88,90). */
enum { EC_PROBE_SIGMOID_BCE = 0, EC_PROBE_SIGMOID_BCE_GATHER = 1, EC_PROBE_SOFTMAX_CE2 = 2 };
int ec_probe_head(int mode, const float* logits, const int64_t* labels, const int64_t* idx, int R, int C,
                  int label_clamp, float* pred, float* dlogits, float* dbias, double* out5, ec_stream_t stream);
/* nn.AdaptiveAvgPool2d((3,3)) (train.py:45) of the cached fp32 NCHW conv features [B,C,H,W] ->
 * rows [B*9, C] so the Conv1x1 (train.py:46) is a row GEMM whose [B*9,52] output equals
 * y_pred.permute(0,2,1).flatten(1) (train.py:70). */
int ec_probe_pool3(const float* conv_nchw, float* rows, int B, int C, int H, int W, ec_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EC_AMD_H */
