/*
 * aq_engine.h -- C ABI of the MI355X-native YOLOv5 detect path (libaqengine.so).
 *
 * What it replaces.  The reference runs the path as a shell command,
 *     python3 yolov5/detect.py --weights W --source DIR --nosave --save-txt --save-conf
 * (reference README.md:77); there is no FFI in the reference for it, and the code it
 * runs is the un-vendored ultralytics/yolov5 submodule (/root/reference/yolov5/yolov5
 * is empty).  The two operator seams inside that script where a native engine plugs
 * in are [UPSTREAM detect.py run()]:
 *     S1  pred = model(im)                      float[B,3,H,W] -> float[B, N, 5+nc]
 *     S2  pred = non_max_suppression(pred, conf_thres, iou_thres, classes, agnostic, max_det)
 * aq_engine_infer() is S1+S2 fused (uint8 tiles in, per-tile detections out);
 * aq_engine_forward_raw() is S1 alone; aq_nms() is S2 alone; the remaining entry points
 * are the individual kernels, exported so each one can be parity-tested by itself.
 *
 * Conventions.
 *   - plain C, pointers and sizes only; every *_dev pointer is device (HBM) memory owned by
 *     the caller; nothing here allocates in a launch path (hipGraph-capture safe).
 *   - all work is enqueued on the hipStream_t passed in (as void*), no host sync.
 *   - return 0 (AQ_OK) or a negative aq_status; aq_last_error() gives a thread-local message.
 *   - activations are NHWC; a tensor argument is (base pointer, pixel stride in elements,
 *     first channel): channel slices of wider buffers are first-class (free Concat).
 */
#ifndef AQ_ENGINE_H
#define AQ_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum aq_status {
    AQ_OK = 0,
    AQ_ERR_INVALID = -1,     /* bad argument / unsupported shape */
    AQ_ERR_HIP = -2,         /* a HIP runtime call failed */
    AQ_ERR_NOMEM = -3,
    AQ_ERR_WORKSPACE = -4    /* workspace too small */
} aq_status;

typedef enum aq_precision {
    AQ_BF16 = 0,   /* bf16 weights + activations, fp32 accumulate/epilogue/head (throughput mode) */
    AQ_FP32 = 1,   /* fp32 everywhere on f32-input MFMA (parity mode: detect.py without --half) */
    AQ_BF16_W8 = 2,/* AQ_BF16 whose conv weights lie on an OCP e4m3fn x 2^e[cout] grid (BASELINE.json configs[3], "fp8 weights"):
                    * kernels that have an fp8-weight stream (the planar 3x3) load the 1-byte codes, the others the same values as bf16 */
    AQ_F16X3 = 3   /* fp32 activations, epilogues and head as AQ_FP32; every conv product as THREE fp16 MFMAs on hi / lo halves of both
                    * operands (22 significant bits each, fp32 accumulate): fp32-grade results at several times the f32-input MFMA's
                    * rate -- the fast parity mode (north_star: boxes / conf within 1e-4 of detect.py's fp32 output).  Domain: activations
                    * within fp16's range (|x| < 65504), as upstream's own --half. */
} aq_precision;

typedef enum aq_op_kind {
    AQ_OP_PREPROCESS = 0, AQ_OP_CONV = 1, AQ_OP_SPPF_POOL = 2, AQ_OP_UPSAMPLE2X = 3,
    AQ_OP_DECODE = 4, AQ_OP_NMS = 5, AQ_OP_STEM = 6, AQ_OP_BOTTLENECK = 7, AQ_OP_DOWNBLOCK = 8
} aq_op_kind;

typedef enum aq_tensor_dtype { AQ_T_ACT = 0, AQ_T_F32 = 1, AQ_T_U8 = 2 } aq_tensor_dtype;

/* One HBM buffer of the plan: NHWC, `channels` contiguous, spatial = (H/down, W/down). */
typedef struct aq_tensor_desc {
    int32_t channels;
    int32_t down;
    int32_t dtype;            /* aq_tensor_dtype */
} aq_tensor_desc;

typedef struct aq_slice { int32_t tensor, ch_off, channels; } aq_slice;

/* One step of the plan (see aquaculture_amd/spec.py for how the YOLOv5 graph is flattened). */
typedef struct aq_op_desc {
    int32_t kind;             /* aq_op_kind */
    aq_slice src, dst, res;   /* res.tensor < 0: no residual */
    int32_t k, stride, pad;
    int32_t act;              /* 1 = SiLU, 0 = identity */
    int32_t level;            /* detect level of a head conv, else -1 */
    const float* weight;      /* host, fp32, KRSC [cout][k][k][cin], BN already folded */
    const float* bias;        /* host, fp32 [cout] */
    double flops_per_tile;    /* algorithmic FLOPs of this op for one tile (reporting only) */
} aq_op_desc;

typedef struct aq_model_desc {
    int32_t precision;        /* aq_precision */
    int32_t nc, na, nl;       /* classes, anchors per level, levels (3) */
    float anchors_px[3][8][2];/* anchor_grid = anchors * stride, pixels, [level][anchor][w,h] */
    float stride[3];
    int32_t head_tensor[3];   /* plan tensor ids of the raw fp32 head maps */
    int32_t input_tensor;     /* plan tensor id of the u8 tiles */
    int32_t n_tensors, n_ops;
    const aq_tensor_desc* tensors;
    const aq_op_desc* ops;
} aq_model_desc;

/* One output detection, in network-input pixels (before scale_boxes), as NMS returns it:
 * [UPSTREAM non_max_suppression] rows (x1, y1, x2, y2, conf, cls). */
typedef struct aq_det { float x1, y1, x2, y2, conf, cls; } aq_det;

typedef struct aq_engine aq_engine;

const char* aq_last_error(void);
int aq_version(void);

/* ---- engine (S1 + S2) ---------------------------------------------------------------- */
/* Copies + packs the weights to the device (the only allocation the engine ever does).  nl = 3, 1 <= na <= 8 and 1 <= nc <= 128 (the two
   64-bit words of the NMS class filter); anything else is AQ_ERR_INVALID and no engine. */
int aq_engine_create(const aq_model_desc* desc, int device_ordinal, aq_engine** out);
void aq_engine_destroy(aq_engine* e);
/* Bytes of caller-provided workspace needed for batches up to max_batch of HxW tiles.  Refuses (AQ_ERR_INVALID, nothing allocated) a batch
 * that some plan op cannot run -- a kernel's size guard with no fallback form, checked with the launchers' own predicates -- with a
 * message naming the op ("plan op N") and the largest batch that fits. */
int aq_engine_workspace_bytes(aq_engine* e, int max_batch, int H, int W, size_t* bytes);
/* Test hook: one size-guard predicate of csrc/size_guards.h (the launchers' and the sizing call's limits) on the n values v, in the
 * order of the function's arguments.  1: fits, 0: refused, -1: unknown `which` or wrong n.  Host arithmetic; needs no GPU. */
enum aq_size_guard_id {
    AQ_SG_PREPROCESS = 0,          /* B, H, W */
    AQ_SG_SPPF_POOL = 1,           /* B, H, W, groups */
    AQ_SG_UPSAMPLE2X = 2,          /* B, H, W, groups */
    AQ_SG_UPSAMPLE2X_ROWS = 3,     /* B, H */
    AQ_SG_STEM = 4,                /* B, H, W */
    AQ_SG_DOWNBLOCK = 5,           /* B, H, W */
    AQ_SG_CONV3X3S2_DIRECT = 6,    /* B, H, W */
    AQ_SG_BOTTLENECK = 7,          /* C, B, H, W */
    AQ_SG_BTL_ASM_TILES = 8,       /* C, B, H, W, in_ld, out_ld */
    AQ_SG_C3TAIL_CAT = 9,          /* B, H, W, cat_ld */
    AQ_SG_CONV1X1_DIRECT = 10,     /* npix */
    AQ_SG_CONV1X1_ASM = 11,        /* npix, in_ld, out_ld */
    AQ_SG_PL3X3_INDEX = 12,        /* B, H, W */
    AQ_SG_PL3X3_OFFSETS = 13,      /* B, H, W, out_ld, res_ld */
    AQ_SG_PL3X3S2 = 14,            /* B, H, W, in_ld, out_ld */
    AQ_SG_PL3X3_F8_OFFSETS = 15,   /* B, H, W, in_ld_bytes, out_ld, res_ld */
    AQ_SG_IGEMM = 16,              /* npix, kgroups_pad, G, cout, bm, bn */
    AQ_SG_HEAD_DECODE = 17,        /* B, ny, nx */
    AQ_SG_TILE_BYTES = 18          /* B, H, W */
};
int aq_size_guard(int which, const long long* v, int n);
/* tiles_dev: uint8 [B][H][W][3] RGB.  dets_dev: [B][max_det].  counts_dev: [B].
 * Replaces `pred = model(im); pred = non_max_suppression(pred, conf, iou, None, False, max_det)`. */
int aq_engine_infer(aq_engine* e, const uint8_t* tiles_dev, int B, int H, int W,
                    void* workspace_dev, size_t workspace_bytes,
                    aq_det* dets_dev, int32_t* counts_dev,
                    float conf_thres, float iou_thres, int max_det, void* stream);
/* S1 only: pred_dev float [B][N][5+nc] (xywh px, obj, cls) exactly as Detect.forward returns it. */
int aq_engine_forward_raw(aq_engine* e, const uint8_t* tiles_dev, int B, int H, int W,
                          void* workspace_dev, size_t workspace_bytes, float* pred_dev, void* stream);
/* Test hook: plan ops [first, last) of aq_engine_infer on the same arguments.  Stepping through the plan in pieces (first = 0 up to
 * aq_engine_num_ops, each piece on the same workspace and stream, in order) launches exactly the kernels, tuned configurations and grids
 * one aq_engine_infer call launches, and writes the same detections and counts once the last op has run. */
int aq_engine_run_ops(aq_engine* e, const uint8_t* tiles_dev, int B, int H, int W, void* workspace_dev, size_t workspace_bytes,
                      int first, int last, float conf_thres, float iou_thres, int max_det, aq_det* dets_dev, int32_t* counts_dev,
                      void* stream);
/* Test hook: device address + geometry of plan tensor `tensor` inside the workspace of the last call. */
int aq_engine_tensor_ptr(aq_engine* e, int tensor, void** ptr, int* channels, int* h, int* w, int* elem_bytes);
/* Per-op device timing with HIP events on the launch stream (bench.py roofline).  ring = number of
 * infer calls whose events are kept; aq_engine_op_times returns mean ms per op over recorded calls. */
int aq_engine_profile(aq_engine* e, int enable, int ring);
/* Test hook: the candidate list the NMS step reads, inside the workspace of the last call: cand int32 [B][cap] (candidate index,
 * level-major as in pred), rows float [B][cap][5+nc] (decoded xywh px, obj, cls) in the same order, counts int32 [B]; cap = N. */
int aq_engine_candidates(aq_engine* e, void** cand_dev, void** rows_dev, void** counts_dev, int* cap);
int aq_engine_op_times(aq_engine* e, float* ms_out, int n_ops, int* calls_recorded);
int aq_engine_num_ops(aq_engine* e);
/* Tuning hook: force the tile configuration of one conv op (-1 = built-in heuristic). */
int aq_engine_set_conv_config(aq_engine* e, int op, int cfg);
/* Tuning: time every tile configuration of every conv op on real activations of a (B,H,W) batch and keep the
 * fastest per op for that geometry (cudnn.benchmark-style).  Synchronises the stream; call once before timing. */
int aq_engine_autotune(aq_engine* e, const uint8_t* tiles_dev, int B, int H, int W,
                       void* workspace_dev, size_t workspace_bytes, int reps, void* stream);
/* fp8 path of BASELINE.json configs[3] (a bf16 engine whose wide Bottleneck 3x3 layers run on the fp8 MFMA, both operands e4m3):
 * 1. aq_engine_calibrate_amax: one bf16 forward pass over calibration tiles; amax_host[i] = max |output| of conv op i (0 for other ops).
 * 2. aq_engine_set_fp8_scales: act_scale[i] > 0 switches conv op i (a 3x3 / stride-1 layer with a planar form, cin % 64 == 0) to
 *    aq_conv3x3_pl_f8 and the 1x1 layer that writes its input to the code-writing epilogue (aq_conv1x1_direct_f8out); act_scale[i] is the
 *    e4m3 scale of that input tensor (value = code x scale; typically amax of the producer / 448).  The pair falls back to bf16 for batch
 *    geometries the fp8 kernel cannot tile.  Weights are quantised per output channel (max |w| / 448) by the packer. */
int aq_engine_calibrate_amax(aq_engine* e, const uint8_t* tiles_dev, int B, int H, int W, void* workspace_dev, size_t workspace_bytes,
                             float* amax_host, int n_ops, void* stream);
int aq_engine_set_fp8_scales(aq_engine* e, const float* act_scale, int n_ops);
int aq_engine_get_conv_config(aq_engine* e, int op);
/* Which kernel family op `op` went to in its most recent launch, and with which tile-configuration id (-1 where none applies): how a
 * test asserts that a layer did not silently fall back -- an fp8 pair to bf16 at another batch size, a planar layer to the implicit-GEMM
 * kernel.  AQ_FAM_NONE before the op's first launch and for pointwise ops. */
enum {
    AQ_FAM_NONE = 0,
    AQ_FAM_IGEMM_OR_HALO = 1,      /* conv_igemm_kernel / conv3x3_halo_kernel; *cfg = tile-shape id (aq_conv_config_tiles) */
    AQ_FAM_PL3X3 = 2,              /* planar 3x3/s1 (generated assembly or the HIP-source build; aq_conv3x3_pl_asm_family names it) */
    AQ_FAM_PL3X3_W8 = 3,           /* the same with the e4m3 weight stream */
    AQ_FAM_PL3X3S2 = 4,            /* planar 3x3/s2 */
    AQ_FAM_PL3X3_F8 = 5,           /* fp8 x fp8 planar 3x3/s1 (consumer of an fp8 pair) */
    AQ_FAM_DIRECT1X1 = 6,
    AQ_FAM_DIRECT1X1_F8OUT = 7,    /* producer of an fp8 pair: writes e4m3 codes */
    AQ_FAM_DIRECT3X3S2 = 8,
    AQ_FAM_BOTTLENECK = 9,         /* *cfg = 1: generated-assembly build (or the C3 tail launch), 0: HIP-source build (aq_bottleneck_asm_form) */
    AQ_FAM_DOWNBLOCK = 10,
    AQ_FAM_STEM = 11,
    AQ_FAM_HEAD_DECODE = 12,
    AQ_FAM_ASM1X1 = 13             /* wide 1x1 in generated assembly (conv1x1_asm_nb13) */
};
int aq_engine_last_launch(aq_engine* e, int op, int* family, int* cfg);
/* Install a table that aq_engine_autotune produced earlier (or on another rank) for the SAME engine and (B,H,W): cfgs[n_ops], one id per
 * op as aq_engine_get_conv_config returns them (-1 for ops that are not tuned).  Used for every batch of that tile geometry (H, W),
 * whatever its size -- a ragged last batch runs the same kernels as the full ones --; geometries without a table keep the built-in
 * heuristic.  The engine holds one table per geometry (each pass of an augmented call uses its own); installing or tuning a geometry
 * replaces that geometry's table only, and aq_engine_get_conv_config reports the most recently installed one.  Ids are validated per op. */
int aq_engine_set_tuned_table(aq_engine* e, int B, int H, int W, const int* cfgs, int n_ops);
int aq_conv_num_configs(void);
/* Diagnostics: arm (buf != NULL) or disarm a device buffer that the STAMPED builds of a few conv tile shapes fill with
 * per-wave phase cycle sums (8 x uint64 per wave); used by tools/stamp_conv.py only. */
int aq_debug_conv_stamp(void* buf_dev, size_t bytes);
/* Diagnostics: register-only bf16 MFMA loop (blocks x 4 waves x iters x 8 MFMAs) to read the sustained matrix rate. */
int aq_debug_mfma_peak(int blocks, int iters, void* out_dev, void* stream);
int aq_conv_config_tiles(int cfg, int* bm, int* bn);

/* ---- individual kernels --------------------------------------------------------------- */
/* Packs fp32 KRSC host weights into the device layout conv kernels read:
 * [cout_pad][k_pad] elements of `precision`, k = (ky, kx, cin) flattened, zero padded.  Returns the
 * byte count via *bytes when packed_dev == NULL.  cout_pad = cout + 384 rounded up to 32: a tile of
 * any configuration (up to 384 rows) reads whole rows, so the rows behind cout are there and zero.
 * aq_conv2d's bias_dev holds as many floats, zero behind cout, for the same reason. */
int aq_pack_conv_weights(const float* w_krsc_host, int cout, int k, int cin, int precision,
                         void* packed_dev, size_t* bytes, void* stream);
/* Implicit-GEMM convolution, NHWC, fused bias + SiLU + residual.  in/out/res element type = precision
 * (out is fp32 when out_f32 != 0).  Replaces Conv.forward_fuse / Bottleneck.forward of the reference's
 * yolov5 dependency [UPSTREAM models/common.py]. */
/* AQ_F16X3 packing: weights as fp16 hi / lo halves of w * 2^s[cout] (s: the power of two that puts the row's largest weight in
 * [2^14, 2^15)), per 8 channels 16 bytes of hi then 16 bytes of lo; bias_scale_dev receives float[2 * rows]: bias * 2^s, then 2^-s
 * (rows = *bias_floats / 2, the padded row count).  aq_conv2d with precision AQ_F16X3 takes THAT buffer as bias_dev.  cin % 8 == 0. */
int aq_pack_conv_weights_x3(const float* w_krsc_host, const float* bias_host, int cout, int k, int cin, void* packed_dev, size_t* bytes,
                            float* bias_scale_dev, size_t* bias_floats, void* stream);
int aq_conv2d(const void* in_dev, int in_ld, int in_choff, int cin,
              void* out_dev, int out_ld, int out_choff, int cout,
              const void* res_dev, int res_ld, int res_choff,
              const void* packed_w_dev, const float* bias_dev,
              int B, int H, int W, int k, int stride, int pad, int act,
              int precision, int out_f32, const void* zero_page_dev, void* stream);
/* Fused stem: uint8 RGB tiles [B][H][W][3] -> x/255 -> Conv(3, cout, k=6, s=2, p=2) + bias + SiLU -> NHWC [B][H/2][W/2][cout slice].
 * Replaces `im.float() / 255` + model.0 of the reference's yolov5 dependency [UPSTREAM detect.py, models/common.py Conv].
 * packed_w_dev comes from aq_pack_stem_weights (fp32 KRSC (cout, 6, 6, 3), BN folded); cout <= 64, H % 4 == 0, W even. */
int aq_pack_stem_weights(const float* w_krsc_host, int cout, int precision, void* packed_dev, size_t* bytes, void* stream);
int aq_stem_conv(const uint8_t* tiles_dev, void* out_dev, int out_ld, int out_choff, int cout, const void* packed_w_dev,
                 const float* bias_dev, int B, int H, int W, int act, int precision, void* stream);

/* Fused Bottleneck (bf16 only, C = 16, 32, 48, 64 or 96): y = (x +) SiLU(cv2_3x3(SiLU(cv1_1x1(x)))) in ONE launch, t never leaves the
 * chip.  Replaces [UPSTREAM models/common.py Bottleneck.forward] for the C3 stages whose hidden width fits
 * (yolov5m: model.2, model.4, model.17).
 * In the plan (op kind AQ_OP_BOTTLENECK): weight = cv1 KRSC [C][1][1][C] followed by cv2 KRSC [C][3][3][C]; bias = b1 | b2.
 * in/out: NHWC [B][H][W][ld] bf16 with the C channels at ch_off; out must not overlap in (neighbour tiles read halos). */
int aq_pack_bottleneck_weights(const float* w1_host, const float* w2_host, int C, void* packed_dev, size_t* bytes, void* stream);
int aq_bottleneck(const void* in_dev, int in_ld, int in_choff, void* out_dev, int out_ld, int out_choff, int C,
                  const void* packed_w_dev, const float* bias_dev, int B, int H, int W, int shortcut, void* stream);
/* Which build aq_bottleneck runs for this launch: 1 = generated assembly (C = 48 or 96; 16 x 16 / 8 x 16 tiles, 32-bit buffer offsets:
 * input under 2^30 bytes, output under 2^31), 0 = the HIP-source kernel (every other launch: AQ_BTL_ASM=0, AQ_BTL96_ASM=0, larger
 * batches, images narrower than two tiles).  Both compute the same operation; they need not round alike. */
int aq_bottleneck_asm_form(int C, int B, int H, int W, int in_ld, int out_ld);

/* A C3 block's last Bottleneck (C = 48) with the block's cv3 1x1 in its epilogue (AQ_OP_BOTTLENECK followed by its AQ_OP_CONV; engines do
 * this on their own, AQ_C3TAIL=0 turns it off): out = SiLU(W3 [Bottleneck(x) | cat] + b3), 96 channels; the Bottleneck's output is not
 * written.  cat: cv2's 48 channels at cat_choff.  bias_dev: b1 | b2 | b3 (192 floats); w3: fp32 KRSC [96][1][1][96].  Bit-identical to
 * aq_bottleneck followed by aq_conv1x1_direct.  Unsupported geometries (the assembly kernel's: images narrower than two tiles,
 * AQ_BTL_ASM=0, 32-bit offsets) return AQ_ERR_INVALID without a launch; aq_bottleneck_c3tail_supported asks first. */
int aq_bottleneck_c3tail_supported(int B, int H, int W, int in_ld, int cat_ld, int out_ld);
int aq_pack_bottleneck_c3tail_weights(const float* w1_host, const float* w2_host, const float* w3_host, void* packed_dev, size_t* bytes,
                                      void* stream);
int aq_bottleneck_c3tail(const void* in_dev, int in_ld, int in_choff, const void* cat_dev, int cat_ld, int cat_choff, void* out_dev,
                         int out_ld, int out_choff, const void* packed_w_dev, const float* bias_dev, int B, int H, int W, int shortcut,
                         void* stream);

/* Fused down-sampling block (bf16 only, 48 -> 96 -> 96 channels): y = SiLU(Wb_1x1 . SiLU(Wa_3x3/s2 (*) x)) in ONE launch.
 * Replaces yolov5m's model.1 = Conv(48, 96, 3, 2) followed by the stacked model.2.cv1|cv2 1x1 convs
 * [UPSTREAM models/common.py Conv.forward_fuse, C3.forward].  In the plan (op kind AQ_OP_DOWNBLOCK): weight = wa KRSC
 * [96][3][3][48] followed by wb KRSC [96][1][1][96]; bias = ba | bb.  in: NHWC [B][H][W][ld]; out: [B][H/2][W/2][ld]. */
int aq_pack_downblock_weights(const float* wa_host, const float* wb_host, void* packed_dev, size_t* bytes, void* stream);
int aq_downblock(const void* in_dev, int in_ld, int in_choff, void* out_dev, int out_ld, int out_choff,
                 const void* packed_w_dev, const float* bias_dev, int B, int H, int W, void* stream);
/* The fused stem in front of it as well (yolov5m model.0 + model.1 + model.2.cv1|cv2 in ONE launch, bf16): the 17 x 33-pixel patch of
 * stem outputs a down-block tile needs is computed from the uint8 tile inside the kernel, so the stem's output tensor (629 MB per
 * 64-tile batch) is never written or read.  Takes exactly aq_stem_conv's and aq_downblock's weight images; bit-identical to the two
 * launches.  Hi, Wi: tile size (multiples of 4). */
int aq_stemdown_supported(int Hi, int Wi);
int aq_stemdown(const uint8_t* tiles_dev, void* out_dev, int out_ld, int out_choff, const void* stem_w_dev, const float* stem_bias_dev,
                const void* packed_w_dev, const float* bias_dev, int B, int Hi, int Wi, void* stream);

/* Direct 1x1 convolution (bf16; Cin -> Cout in {96->96, 192->192, 384->192, 384->384}): no K pipeline, whole-K pixel tiles by LDS-DMA, weights
 * in registers.  Same operation as aq_conv2d with k = 1; the engine's autotuner times it per layer against the implicit-GEMM tile
 * shapes under the config id AQ_CONV_CFG_DIRECT1X1. */
#define AQ_CONV_CFG_DIRECT1X1 1000
/* OR-ed into a tile configuration id (aq_conv2d, aq_engine_set_conv_config): launch one workgroup per output tile instead of the
 * persistent grid (one or two resident workgroups per CU striding over the tiles).  Tiles then reach CUs in the order CUs become
 * free; the autotuner times both forms per layer. */
#define AQ_CONV_CFG_ONE_TILE_PER_WG 4096
int aq_conv1x1_direct_supported(int cin, int cout);
int aq_pack_conv1x1_direct(const float* w_host, int cin, int cout, void* packed_dev, size_t* bytes, void* stream);
int aq_conv1x1_direct(const void* in_dev, int in_ld, int in_choff, void* out_dev, int out_ld, int out_choff, int cin, int cout,
                      const void* packed_w_dev, const float* bias_dev, long long npix, int act, void* stream);

/* Wide 1x1 convolution in generated gfx950 assembly (bf16, SiLU; Cin a multiple of 96, Cout in {384, 768, 1536}: yolov5m's K >= 768 1x1 layers --
 * C3 cv1|cv2 / cv3 at 20x20, SPPF cv1 / cv2, model.10, model.13 cv1|cv2).  208-pixel x 384-channel tiles, eight waves, weights streamed from L2
 * to registers, pixels by buffer-descriptor LDS-DMA in 96-channel chunks (csrc/gen_conv1x1_asm.py).  Same operation as aq_conv2d with k = 1,
 * act = 1; autotuner candidate AQ_CONV_CFG_ASM1X1.  npix: pixels (B x H x W); in / out may be channel slices of wider tensors. */
#define AQ_CONV_CFG_ASM1X1 1004
int aq_conv1x1_asm_supported(int cin, int cout);
int aq_pack_conv1x1_asm(const float* w_host, int cin, int cout, void* packed_dev, size_t* bytes, void* stream);
int aq_conv1x1_asm(const void* in_dev, int in_ld, int in_choff, void* out_dev, int out_ld, int out_choff, int cin, int cout,
                   const void* packed_w_dev, const float* bias_dev, long long npix, int act, void* stream);

/* Direct 3x3 / stride 2 / pad 1 convolution (bf16; 96 -> 192 channels: yolov5m's model.3), the plain form of the down-block kernel:
 * input patches by LDS-DMA, weights in registers (last k-steps in LDS), each input-row fragment loaded once for the output rows it
 * serves.  Autotuner candidate AQ_CONV_CFG_DIRECT3X3S2. */
#define AQ_CONV_CFG_DIRECT3X3S2 1001
int aq_conv3x3s2_direct_supported(int cin, int cout);
int aq_pack_conv3x3s2_direct(const float* w_host, int cin, int cout, void* packed_dev, size_t* bytes, void* stream);
int aq_conv3x3s2_direct(const void* in_dev, int in_ld, int in_choff, void* out_dev, int out_ld, int out_choff, int cin, int cout,
                        const void* packed_w_dev, const float* bias_dev, int B, int H, int W, int act, void* stream);
/* 3x3 / stride 1 / pad 1 convolution of the wide Bottleneck layers (bf16; Cin a multiple of 64 and >= 128, Cout a multiple of 192:
 * yolov5m's 192 -> 192 and 384 -> 384 [UPSTREAM models/common.py Bottleneck.cv2]): four waves, one per SIMD, weights streamed from L2
 * straight into registers in MFMA-fragment order (aq_pack_conv3x3_pl), the input region staged in LDS as padded, slot-major planes
 * (conflict-free fragment reads for every tap with no masks), a three-buffer chunk ring with ONE workgroup barrier per 64-channel chunk.
 * (Round 3: on 20- and 40-pixel-wide images -- yolov5m's two widths -- the region is staged as 64-byte pixel-major rows through a buffer
 * descriptor instead, a quarter of the cache-line look-ups per LDS-DMA instruction; same tiles, packed weights and results.)
 * Same operation as aq_conv2d with k = 3, stride = 1, pad = 1; the engine's autotuner times it per layer under AQ_CONV_CFG_PL3X3.
 * in_dev: first channel of the input; element (pixel P, 16-byte channel group g) lives at in_dev + P * in_pixel_stride_b +
 * g * in_group_stride_b (NHWC: row bytes and 16).  out / res: NHWC bf16 slices as in aq_conv2d (res may alias out: in-place shortcut). */
#define AQ_CONV_CFG_PL3X3 1002
int aq_conv3x3_pl_supported(int cin, int cout);
/* 1 when the assembly family with `nb` 16-pixel blocks per tile is part of this build (13: always; 7, 8: two workgroups per CU, an
 * experiment that wins on no BASELINE geometry, built only with AQ_GEN_EXPERIMENTAL=1), else 0; negative aq_status on a HIP error. */
int aq_conv3x3_pl_asm_family(int nb);
int aq_pack_conv3x3_pl(const float* w_krsc_host, int cin, int cout, void* packed_dev, size_t* bytes, void* stream);
int aq_conv3x3_pl(const void* in_dev, long long in_pixel_stride_b, long long in_group_stride_b, int cin,
                  void* out_dev, int out_ld, int out_choff, int cout, const void* res_dev, int res_ld, int res_choff,
                  const void* packed_w_dev, const float* bias_dev, int B, int H, int W, int act, void* stream);
/* 3x3 / stride 2 / pad 1 on the same planar scheme (round 3; bf16, Cin a multiple of 32 and >= 64, Cout a multiple of 192 with Cout / 192 a
 * power of two, even H and W, and an output row short enough for the tile's region: yolov5m's model.5 / 7 / 18 / 21, i.e.
 * [UPSTREAM models/common.py Conv.forward_fuse] with k = 3, s = 2): the input region is staged in LDS as the four PARITY planes of the
 * input (y, x odd / even), each in padded OUTPUT coordinates, so a tap is a plane plus an offset of -1 or 0 and every fragment read
 * stays conflict-free; 32-channel chunks, two ring buffers, one barrier per chunk, weights L2 -> registers.  Generated gfx950 assembly
 * (csrc/gen_conv3x3_pl_asm.py, family s2nb13).  Same operation as aq_conv2d with k = 3, stride = 2, pad = 1; autotuner candidate
 * AQ_CONV_CFG_PL3X3S2.  H, W: the INPUT's size. */
#define AQ_CONV_CFG_PL3X3S2 1003
int aq_conv3x3_pl_s2_supported(int cin, int cout, int B, int H, int W);
int aq_pack_conv3x3_pl_s2(const float* w_krsc_host, int cin, int cout, void* packed_dev, size_t* bytes, void* stream);
int aq_conv3x3_pl_s2(const void* in_dev, int in_ld, int in_choff, int cin, void* out_dev, int out_ld, int out_choff, int cout,
                     const void* packed_w_dev, const float* bias_dev, int B, int H, int W, int act, void* stream);
/* fp8 on BOTH MFMA operands (round 3; BASELINE.json configs[3]): the stride-1 planar kernel on v_mfma_f32_16x16x128_f8f6f4 -- input tensor =
 * OCP e4m3fn codes (NHWC, one byte per channel, value = code x act_scale, written by the producing kernel), weights quantised by the
 * packer with one scale per output channel (max |w| / 448), fp32 accumulate, epilogue x act_scale x w_scale[co] + bias, SiLU, shortcut,
 * bf16 out.  cin a multiple of 64, cout of 192 (cout / 192 a power of two).  in_ld / in_choff in BYTES (= channels). */
int aq_conv1x1_direct_f8out(const void* in_dev, int in_ld, int in_choff, void* out_dev, int out_pitch_bytes, int out_byte_off, int cin, int cout,
                            const void* packed_w_dev, const float* bias_dev, long long npix, int act, float out_scale, void* stream);
int aq_absmax_bf16(const void* t_dev, int ld, int choff, int c, long long npix, float* out_dev, void* stream);
unsigned char aq_f32_to_e4m3(float v);      /* round to nearest even, saturating at +-448 */
int aq_conv3x3_pl_f8_supported(int cin, int cout, int B, int H, int W);
int aq_pack_conv3x3_pl_f8(const float* w_krsc_host, const float* bias_host, int cin, int cout, float act_scale, void* packed_dev,
                          size_t* bytes, float* scale_bias_dev, void* stream);
int aq_conv3x3_pl_f8(const void* in_dev, int in_ld, int in_choff, int cin, void* out_dev, int out_ld, int out_choff, int cout,
                     const void* res_dev, int res_ld, int res_choff, const void* packed_w_dev, const float* scale_bias_dev,
                     int B, int H, int W, int act, void* stream);
/* The same kernel streaming e4m3fn weight codes (AQ_BF16_W8): bit-identical outputs to aq_conv3x3_pl on the dequantised weights.
 * `w` must lie on a per-output-channel grid code x 2^e (AQ_ERR_INVALID otherwise); scale_bias_dev: float[2048] written by the packer
 * (bias x 2^-e, then 2^e).  _supported: NB = 13 tiles fit the image and cout / 192 is a power of two. */
int aq_conv3x3_pl_w8_supported(int cin, int cout, int B, int H, int W);
int aq_pack_conv3x3_pl_w8(const float* w_krsc_host, const float* bias_host, int cin, int cout, void* packed_dev, size_t* bytes,
                          float* scale_bias_dev, void* stream);
int aq_conv3x3_pl_w8(const void* in_dev, long long in_sp, long long in_ss, int cin, void* out_dev, int out_ld, int out_choff,
                     int cout, const void* res_dev, int res_ld, int res_choff, const void* packed_w8_dev,
                     const float* scale_bias_dev, int B, int H, int W, int act, void* stream);
/* uint8 RGB NHWC -> 2x2 space-to-depth, 16 channels, value/255 ([UPSTREAM detect.py: im.float()/255]). */
int aq_preprocess_s2d(const uint8_t* tiles_dev, void* out_dev, int B, int H, int W, int precision, void* stream);
/* Letterbox on device (the real 1024x1024 tiles of reference src/load_data/tile_tifs.py:13 -> 640x640):
 * [UPSTREAM utils/augmentations.py letterbox] = cv2.resize(INTER_LINEAR) to (new_w, new_h) + constant border 114, uint8 RGB NHWC.
 * xtab_dev / ytab_dev: int32 [new_w][4] / [new_h][4] rows (i0, i1, w0, w1): OpenCV's 11-bit fixed-point coefficient tables, built
 * on the host (aquaculture_amd/dataloader.py resize tables).  UNPINNED: no OpenCV is available to check against. */
int aq_letterbox_u8(const uint8_t* src_dev, int B, int H0, int W0, uint8_t* dst_dev, int H, int W, int new_w, int new_h,
                    int top, int left, const int32_t* xtab_dev, const int32_t* ytab_dev, void* stream);
/* The same letterbox reading its B tiles (H0 x W0) out of ONE uint8 RGB raster in device memory: tile b starts tile_off[b] bytes into
 * the raster, rows are row_bytes apart.  Replaces the crop + re-encode of reference src/load_data/tile_tifs.py:13-47 (gdal.Translate
 * srcWin per tile) + :50-74 (JPEG) for the opt-in scene mode: the scene is uploaded once and never written back as tiles.  The offsets
 * are passed twice: tile_off_dev for the kernel, tile_off_host so that the call can refuse tiles that leave the raster. */
int aq_letterbox_tiles_u8(const uint8_t* scene_dev, long long scene_bytes, long long row_bytes, const long long* tile_off_dev,
                          const long long* tile_off_host, int B, int H0, int W0, uint8_t* dst_dev, int H, int W, int new_w, int new_h,
                          int top, int left, const int32_t* xtab_dev, const int32_t* ytab_dev, void* stream);
/* Split JPEG decode (round 3): the pixel half of what [UPSTREAM detect.py LoadImages -> cv2.imread] gets from
 * libjpeg(-turbo) -- dequantisation, the islow IDCT, h2v2 fancy chroma upsampling, YCbCr -> RGB -- bit for bit, on the device.  Input: the
 * quantised coefficient blocks of B baseline 4:2:0 JPEGs of one size as written by aq_jpeg_decode_coeffs (libaqjpeg.so, include/aq_jpeg.h:
 * the entropy decoder, which stays on the host), image b from coef_off_dev[b] (int16 units, a multiple of 64), qt_dev uint16 [B][3][64].
 * Output: uint8 RGB [B][H][W][3].  scratch_dev: aq_jpeg_scratch_bytes(B, H, W) bytes.
 * THE ACCEPTANCE RULE: "bit for bit" holds for images all of whose blocks keep every value of the IDCT's pass-1 workspace (the column pass,
 * DESCALEd by 11 bits) within +-AQ_JPEG_WS_MAX -- the rule of oracle/jpeg_oracle.py (WS_MAX; tests/test_jpeg_synth.py ties the two
 * constants and pins the rule to libjpeg-turbo).  Beyond it the library's pixels depend on its build.  aq_jpeg_idct_rgb_checked zeroes
 * flags_dev (int32 [B]) on the stream and sets image b's flag to 1 when one of its blocks is outside the rule; the image's pixels are
 * written all the same and are nobody's.  aq_jpeg_idct_rgb is the checked entry without flags: its pixels are libjpeg's only for
 * accepted blocks, and it cannot say when they are not. */
#define AQ_JPEG_WS_MAX 16383
/* Inside the rule every dequantised coefficient satisfies |coef q| < 4096 (the column pass is invertible with known gains).  The kernel
 * refuses a block beyond this bound BEFORE it looks at its 32-bit workspace, which a larger value can wrap back into range. */
#define AQ_JPEG_DEQ_MAX 4096
size_t aq_jpeg_scratch_bytes(int B, int H, int W);
int aq_jpeg_idct_rgb_checked(const int16_t* coef_dev, const long long* coef_off_dev, const uint16_t* qt_dev, int B, int H, int W,
                             void* scratch_dev, uint8_t* out_dev, int32_t* flags_dev, void* stream);
int aq_jpeg_idct_rgb(const int16_t* coef_dev, const long long* coef_off_dev, const uint16_t* qt_dev, int B, int H, int W,
                     void* scratch_dev, uint8_t* out_dev, void* stream);
/* GPU entropy decode (round 4): the Huffman stage of the same decode on the device, one lane per restart segment (= per image for files
 * without restart markers).  Replaces the host half's aq_jpeg_decode_coeffs ([UPSTREAM LoadImages -> cv2.imread]'s entropy stage;
 * producer of the files: reference src/load_data/tile_tifs.py:66-74).  streams_dev: the bytes aq_jpeg_prepare (include/aq_jpeg.h) wrote,
 * uploaded as they are; segs_dev: nseg descriptors of 32 bytes {u32 stream_off, u32 stream_len, u64 coef_off (int16 index of the image's
 * first coefficient in coef_dev), u32 mcu0, u32 n_mcu, u16 mcu_cols, u16 mcu_rows, u32 tabset}; tabsets_dev: table sets of six
 * aq_jpeg_gpu_tab each; coef_dev: ZEROED coefficient buffers in aq_jpeg_decode_coeffs's layout; status_dev: int32 per segment (0 ok, 2 corrupt).
 * A segment owns [stream_off, stream_off + ((stream_len + 8 + 15) & ~15)): its data plus the zero bytes aq_jpeg_prepare writes behind it.
 * A lane's status and every coefficient it stores depend on owned bytes only: it takes no stream word that ends past stream_len + 8 bytes,
 * and a lane that would need more bits ends with status 2 (the host decoder's rule, "consumed bits the file does not contain", applied
 * when it happens).  The kernel loads the stream in 64-byte chunks from each segment's start, two chunks ahead, so it loads no byte at or
 * past stream_off + stream_len + 8 + 192: streams_dev needs 256 readable bytes behind the last slot, whatever the files hold.  The caller
 * validates every offset; the kernel trusts them. */
int aq_jpeg_huffman_decode(const void* streams_dev, const void* segs_dev, int nseg, const void* tabsets_dev, void* coef_dev,
                           void* status_dev, void* stream);
/* SPPF pools: y1 = mp5(x), y2 = mp5(y1), y3 = mp5(y2) written to channel slices c, 2c, 3c of the same buffer. */
int aq_sppf_pool(void* buf_dev, int ld, int ch_off, int c, int B, int H, int W, int precision, void* stream);
/* nearest 2x upsample of a channel slice into a channel slice. */
int aq_upsample2x(const void* in_dev, int in_ld, int in_choff, void* out_dev, int out_ld, int out_choff,
                  int c, int B, int H, int W, int precision, void* stream);
/* One Detect level fused with its decode (bf16, small heads: na * (nc + 5) <= 32, cin a multiple of 32 up to 1024): the 1x1 head conv,
 * sigmoid(objectness) > conf_thres, box decode and the append to the image's compact candidate list, with the arithmetic of
 * aq_detect_decode; the fp32 head maps are never written.  The caller zeroes the counters before the first level.
 * [UPSTREAM models/yolo.py Detect.forward + utils/general.py non_max_suppression's candidate filter] */
int aq_head_decode_supported(int cin, int na, int nc);
int aq_pack_head_weights(const float* w_host, const float* bias_host, int cin, int cout, void* packed_dev, size_t* bytes, void* stream);
int aq_head_decode(const void* in_dev, int in_ld, int in_choff, int cin, const void* packed_dev, int B, int ny, int nx,
                   int cand_off, float stride, const float* anchors_px, int nc, int na, float conf_thres,
                   int32_t* cand_dev, float* cand_rows_dev, int32_t* cand_count_dev, int count_stride, int cand_cap, void* stream);
/* image b's candidate counter lives at cand_count_dev[b * count_stride] (the engine spaces them 4 KB apart: adjacent counters share an L2
 * channel and its atomic unit); this copies them into the compact [B] array aq_nms reads. */
int aq_head_counts_gather(const int32_t* wide_dev, int count_stride, int32_t* compact_dev, int B, void* stream);

/* Detect.forward inference branch on raw fp32 head maps [B][ny][nx][head_ld] (channel = a*no + o):
 * writes pred [B][N][no] when pred_dev != NULL; when cand_dev != NULL also compacts the candidates with
 * obj > conf_thres: their candidate indices into cand_dev[B][cand_cap], their decoded rows into
 * cand_rows_dev[B][cand_cap][no] (optional) and their number into cand_count_dev[B]. */
int aq_detect_decode(const float* const head_dev[3], int head_ld, int B, int H, int W, int nc, int na,
                     const float* anchors_px /* [3][na][2] host */, const float* stride /* [3] host */,
                     float* pred_dev, float conf_thres, int32_t* cand_dev, float* cand_rows_dev,
                     int32_t* cand_count_dev, int cand_cap, void* stream);
/* S2: non_max_suppression(pred, conf, iou, classes=None, agnostic=False, multi_label=False, max_det).
 * rows_dev is either the full pred [B][N][no] (rows_per_tile = N, cand_dev = NULL) or the compact rows
 * aq_detect_decode wrote (rows_per_tile = cand_cap, with cand_dev / cand_count_dev).
 * scratch_dev: aq_nms_scratch_bytes(B, N).  Deterministic: ties in confidence by ascending candidate index;
 * no wall-clock time limit.  N < 131072. */
size_t aq_nms_scratch_bytes(int B, int N);
int aq_nms(const float* rows_dev, int rows_per_tile, int B, int N, int nc, float conf_thres, float iou_thres,
           int max_det, const int32_t* cand_dev, const int32_t* cand_count_dev, int cand_cap,
           void* scratch_dev, aq_det* dets_dev, int32_t* counts_dev, void* stream);
/* aq_nms with upstream's two other options: agnostic != 0 = class-agnostic suppression (no per-class box offset); classes_lo / classes_hi = bit
 * mask of the classes kept (bit c of lo, bit c - 64 of hi; all ones = no filter), applied after the confidence threshold as upstream's
 * `x[(x[:, 5:6] == classes).any(1)]` [UPSTREAM utils/general.py non_max_suppression(classes, agnostic)]. */
int aq_nms_opts(const float* rows_dev, int rows_per_tile, int B, int N, int nc, float conf_thres, float iou_thres,
                int max_det, const int32_t* cand_dev, const int32_t* cand_count_dev, int cand_cap,
                void* scratch_dev, aq_det* dets_dev, int32_t* counts_dev, int agnostic, unsigned long long classes_lo,
                unsigned long long classes_hi, void* stream);
/* The engine's NMS step (aq_engine_infer) with those options; defaults: agnostic = 0, every class. */
int aq_engine_set_nms_options(aq_engine* e, int agnostic, unsigned long long classes_lo, unsigned long long classes_hi);

/* ---- test-time augmentation (detect.py --augment) -------------------------------------- */
/* [UPSTREAM models/yolo.py DetectionModel._forward_augment]: three passes (scale, flip) = (1, -), (0.83, left-right), (0.67, -) over
 * xi = scale_img(flip(im), s, gs = 32) [UPSTREAM utils/torch_utils.py scale_img]: F.interpolate(bilinear, align_corners = False) to
 * (int(H s), int(W s)), then padded right / bottom with 0.447 to ceil(H s / 32) 32 x ceil(W s / 32) 32.  Each pass's decoded Detect output
 * is de-scaled (xywh / s; x = W - x for the flipped pass) [_descale_pred], the last N_0 // 21 rows of pass 0 and the first
 * 16 (N_2 // 21) rows of pass 2 are dropped [_clip_augmented] -- with H, W multiples of 32 exactly the P5 level of pass 0 and the P3
 * level of pass 2 --, and the passes are concatenated: N_aug rows per image (45147 at 640 x 640, against 25200 for one pass). */
typedef struct aq_augment_pass {
    float scale;
    int32_t flip;              /* 1: left-right flip before scaling */
    int32_t h, w;              /* interpolated size: int(H s), int(W s) */
    int32_t hp, wp;            /* padded size the network runs at (multiples of 32) */
    int32_t rows;              /* rows of the pass's Detect output (na x the three levels at hp x wp) */
    int32_t keep_first, keep_count;   /* rows of the pass that _clip_augmented keeps */
    int32_t out_first;         /* row of the concatenated prediction that row keep_first becomes */
    int32_t level_mask;        /* bit l set: level l survives the clip (its head conv and decode run) */
} aq_augment_pass;
/* The three passes of an H x W tile (H, W positive multiples of 32; na anchors per level); *n_aug = rows per image of the augmented
 * prediction.  The one place the geometry is derived (the engine and the Python side both call it). */
int aq_augment_geometry(int H, int W, int na, aq_augment_pass passes_out[3], int* n_aug);
/* One bilinear tap per output row / column of F.interpolate(align_corners = False) from `in` to `out` samples, in PyTorch's CPU fp32
 * arithmetic: src = max(fmaf(float(in) / out, d + 0.5f, -0.5f), 0) (one rounding, as its build), i0 = (int)src, i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1.
 * flip != 0 mirrors the source indices (in - 1 - i) for a left-right flip done before the interpolation. */
typedef struct aq_tap { int32_t i0, i1; float l0, l1; } aq_tap;
int aq_augment_taps(int in, int out, int flip, aq_tap* taps_host);
/* Scaled-input stem: aq_stem_conv on scale_img(flip(u8 / 255)) without writing that image anywhere.  tiles: uint8 [B][H0][W0][3];
 * ytab_dev / xtab_dev: aq_tap [h] / [w] (aq_augment_taps, the column taps already mirrored for a flipped pass); the network input is
 * hp x wp: interpolated samples inside h x w, 0.447 beyond them, and the stem's own zero padding outside hp x wp.  Each sample is
 * computed in fp32 on the v / 255 values as h0 (w0 x00 + w1 x01) + h1 (w0 x10 + w1 x11) and rounded once to the element type of the
 * precision (fp32, or bf16 RNE).  Same weight image and output layout as aq_stem_conv; hp % 4 == 0, wp even. */
int aq_stem_conv_scaled(const uint8_t* tiles_dev, int H0, int W0, const aq_tap* ytab_dev, const aq_tap* xtab_dev, int h, int w,
                        void* out_dev, int out_ld, int out_choff, int cout, const void* packed_w_dev, const float* bias_dev,
                        int B, int hp, int wp, int act, int precision, void* stream);
/* The same sampling in front of aq_preprocess_s2d (plans without the fused stem): out = space-to-depth of the hp x wp network input. */
int aq_preprocess_s2d_scaled(const uint8_t* tiles_dev, int H0, int W0, const aq_tap* ytab_dev, const aq_tap* xtab_dev, int h, int w,
                             void* out_dev, int B, int hp, int wp, int precision, void* stream);
/* aq_head_decode for one pass of an augmented call: the same arithmetic, then xywh / scale (fp32 division) and, flip_w != 0,
 * x = flip_w - x.  cand_off: row of the concatenated prediction that this level's first candidate becomes.  Appends to the counters;
 * the caller zeroes them once for all three passes. */
int aq_head_decode_aug(const void* in_dev, int in_ld, int in_choff, int cin, const void* packed_dev, int B, int ny, int nx,
                       int cand_off, float stride, const float* anchors_px, int nc, int na, float conf_thres, float scale, float flip_w,
                       int32_t* cand_dev, float* cand_rows_dev, int32_t* cand_count_dev, int count_stride, int cand_cap, void* stream);
/* aq_detect_decode for one pass of an augmented call: H x W = the pass's network input; only levels in level_mask are decoded; pass row n
 * becomes row cand_base + n of the concatenated prediction (pred_dev [B][rows_per_image][no]; cand indices likewise); de-scale as
 * aq_head_decode_aug.  Appends to cand_count_dev (not zeroed here). */
int aq_detect_decode_aug(const float* const head_dev[3], int head_ld, int B, int H, int W, int nc, int na, const float* anchors_px,
                         const float* stride, int level_mask, int cand_base, int rows_per_image, float scale, float flip_w,
                         float* pred_dev, float conf_thres, int32_t* cand_dev, float* cand_rows_dev, int32_t* cand_count_dev,
                         int cand_cap, void* stream);
/* The engine's augmented path: the same arguments as the plain entry points; forward_raw_augment writes pred_dev [B][N_aug][5+nc] in
 * upstream's row order.  Refused (AQ_ERR_INVALID) when N_aug reaches aq_nms's row limit, and on engines with fp8 activation scales. */
int aq_engine_workspace_bytes_augment(aq_engine* e, int max_batch, int H, int W, size_t* bytes);
int aq_engine_infer_augment(aq_engine* e, const uint8_t* tiles_dev, int B, int H, int W, void* workspace_dev, size_t workspace_bytes,
                            aq_det* dets_dev, int32_t* counts_dev, float conf_thres, float iou_thres, int max_det, void* stream);
int aq_engine_forward_raw_augment(aq_engine* e, const uint8_t* tiles_dev, int B, int H, int W, void* workspace_dev,
                                  size_t workspace_bytes, float* pred_dev, void* stream);
/* aq_engine_last_launch for pass `pass` (0..2) of the most recent augmented call. */
int aq_engine_last_launch_augment(aq_engine* e, int pass, int op, int* family, int* cfg);

/* Host helper: n label rows (cls xc yc w h conf, fp32, stride 6) -> the text detect.py --save-txt [--save-conf] writes
 * ("%g" per value, one line per row).  Returns bytes written or -(bytes needed). */
long aq_format_label_rows(const float* rows, int n, int save_conf, char* buf, size_t buflen);
/* A batch of label files per call (no interpreter lock held): tile t's rows are rows[offsets[t] .. offsets[t + 1]); tiles with rows get
 * <dir>/<stems[t]>.txt with aq_format_label_rows's bytes (truncating), tiles without get no file.  Returns files written, or -1 - t. */
long aq_write_label_files(const char* dir, const char* const* stems, const float* rows, const long long* offsets, int n_tiles,
                          int save_conf, int do_fsync);

/* --save-crop [UPSTREAM utils/plots.py save_one_box: Pillow, quality=95, subsampling=0]: one crop of a uint8 RGB image in device memory.
 * Pixel (x, y) of its image is at base + y * pitch + 3 x; the crop is [x1, x2) x [y1, y2); block = its first 8x8 block position in the
 * coefficient arena.  A block position holds 3 x 64 int16 (Y, Cb, Cr), each block in zigzag order; a crop has ceil(w / 8) ceil(h / 8)
 * positions in raster order. */
typedef struct aq_crop { int64_t base; int32_t pitch, x1, y1, x2, y2, block; } aq_crop;
/* Device half of the crop encoder, bit-exact with libjpeg(-turbo) at quality 95, 4:4:4: edge replication, rgb_ycc_convert, level shift,
 * jpeg_fdct_islow, quantisation.  crops_dev: n_crops crops sorted by block, back to back; coef_dev receives n_blocks positions, the first
 * crop's first position at coef_dev.  A crop whose window leaves [images_dev, images_dev + image_bytes) gets zero coefficients. */
int aq_crop_jpeg_coefs(const uint8_t* images_dev, long long image_bytes, const aq_crop* crops_dev, int n_crops, int n_blocks,
                       int16_t* coef_dev, void* stream);
/* Host half: the JFIF file of one w x h crop from its coefficient positions (the markers, tables and entropy coding Pillow's encoder
 * writes).  Returns bytes written, or -(bytes needed). */
long aq_crop_jpeg_bytes(const int16_t* coef, int w, int h, uint8_t* buf, size_t buflen);
/* A batch of crop files on n_threads threads (no interpreter lock held): crop i, coefficients from position crops[i].block of coef (host
 * memory), -> <dir>/<rel_paths[i]> (truncating; missing directories are created).  Returns files written, or -1 - i. */
long aq_write_crop_files(const char* dir, const char* const* rel_paths, const int16_t* coef, const aq_crop* crops, int n_crops,
                         int n_threads, int do_fsync);

/* Annotated images (detect.py without --nosave) [UPSTREAM utils/plots.py Annotator.box_label, Pillow branch; detect.py cv2.imwrite].
 * aq_canvas: one w x h uint8 RGB image of a batch.  Its pixel (x, y) is at src + y * src_pitch + 3 x of the source buffer, the annotated copy at
 * dst + y * dst_pitch + 3 x of the destination buffer; cell = its first 16 x 16-pixel cell in the cell table (ceil(w / 16) ceil(h / 16) cells,
 * raster order), unit = its first draw unit (four cells side by side: ceil(ceil(w / 16) / 4) ceil(h / 16) units).
 * aq_prim: pixels [x0, x1] x [y0, y1] (inclusive, inside the image).  mask_w == 0: filled with rgb (R | G << 8 | B << 16).  mask_w > 0: rgb
 * composited through an 8-bit mask with Pillow's BLEND8; pixel (x, y) reads atlas byte mask + (y - y0) * mask_w + (x - x0). */
typedef struct aq_canvas { int64_t src, dst; int32_t src_pitch, dst_pitch, w, h, cell, unit; } aq_canvas;
typedef struct aq_prim { int32_t x0, y0, x1, y1; uint32_t rgb; int32_t mask_w; int64_t mask; } aq_prim;
/* Out of place, pixel-centric: every pixel of every canvas = its source pixel with the primitives of its cell applied in table order.
 * cell_start_dev: n_cells + 1 ascending offsets into cell_prims_dev (n_entries indices into prims_dev, ascending inside a cell).  canvases_host =
 * canvases_dev's content in host memory: a canvas that leaves a buffer is refused before the launch. */
int aq_annotate_u8(const uint8_t* src_dev, long long src_bytes, uint8_t* dst_dev, long long dst_bytes, const aq_canvas* canvases_dev,
                   const aq_canvas* canvases_host, int n_canvases, const aq_prim* prims_dev, int n_prims, const int32_t* cell_start_dev,
                   int n_cells, const int32_t* cell_prims_dev, int n_entries, const uint8_t* atlas_dev, long long atlas_bytes, void* stream);
/* Whole-frame JPEG, what cv2.imwrite's libjpeg writes for a .jpg: quality 95, 4:2:0, standard Huffman tables; byte-identical to Pillow's
 * save(quality=95, subsampling=2) of the same pixels (OpenCV's own header bytes are not pinned).  aq_frame: a w x h image at base (pixel (x, y)
 * at base + y * pitch + 3 x); mcu = its first 16 x 16 MCU in the coefficient arena.  An MCU holds 6 x 64 int16: Y00 Y01 Y10 Y11 Cb Cr, the
 * interleaved scan's order, each block in zigzag order; a frame has ceil(w / 16) ceil(h / 16) MCUs in raster order. */
typedef struct aq_frame { int64_t base; int32_t pitch, w, h, mcu; } aq_frame;
/* Device half: edge replication, rgb_ycc_convert, h2v2_downsample, level shift, jpeg_fdct_islow, quantisation, libjpeg's dummy blocks.
 * frames: sorted by mcu, back to back; frames_host = the same table in host memory (a frame that leaves the buffer is refused). */
int aq_image_jpeg_coefs(const uint8_t* images_dev, long long image_bytes, const aq_frame* frames_dev, const aq_frame* frames_host, int n_frames,
                        int n_mcus, int16_t* coef_dev, void* stream);
/* Host half, siblings of aq_crop_jpeg_bytes / aq_write_crop_files: one frame's file; a batch of files on n_threads threads. */
long aq_image_jpeg_bytes(const int16_t* coef, int w, int h, uint8_t* buf, size_t buflen);
long aq_write_image_files(const char* dir, const char* const* rel_paths, const int16_t* coef, const aq_frame* frames, int n_frames,
                          int n_threads, int do_fsync);
/* The same three with libjpeg's quality, 1 .. 100 (jpeg_set_quality: Annex K tables scaled by 5000 / q below 50 and 200 - 2 q from there,
 * clamped to [1, 255]; the DQT segments of the file follow): the three above are these at 95.  75 is Pillow's save() default, 4:2:0 with
 * it: aq_image_jpeg_bytes_q(75) is byte-identical to Image.save(f) of the same pixels.  Any other quality is refused (AQ_ERR_INVALID; 0; -1). */
int aq_image_jpeg_coefs_q(const uint8_t* images_dev, long long image_bytes, const aq_frame* frames_dev, const aq_frame* frames_host, int n_frames,
                          int n_mcus, int quality, int16_t* coef_dev, void* stream);
long aq_image_jpeg_bytes_q(const int16_t* coef, int w, int h, int quality, uint8_t* buf, size_t buflen);
long aq_write_image_files_q(const char* dir, const char* const* rel_paths, const int16_t* coef, const aq_frame* frames, int n_frames,
                            int quality, int n_threads, int do_fsync);

/* val.py --plots: the mosaics val_batch{i}_labels.jpg / val_batch{i}_pred.jpg [UPSTREAM utils/plots.py plot_images, output_to_target; val.py].
 * Grid: the first n = min(B, 16) letterboxed network inputs of a batch (uint8 RGB, H x W), ns = ceil(sqrt(n)); image i has its origin at
 *   (x, y) = (W (i / ns), H (i % ns)) -- column-major -- of a white (255) ns H x ns W source mosaic.  scale = max_size / ns / max(H, W),
 *   max_size = 1920.  scale < 1: h = ceil(scale H), w = ceil(scale W) and the mosaic is cv2.resize()d (INTER_LINEAR) to (w ns, h ns), the x
 *   and y ratios being ns W / (ns w) and ns H / (ns h) (not 1 / scale); otherwise h = H, w = W and the mosaic is the paste itself.
 * Pixels: the uint8 letterboxed pixels themselves (upstream pastes (im / 255) * 255 truncated, which loses a count on some values).
 * Annotation, all through Annotator(pil=True)'s rules as aq_annotate_u8 draws them: fs = int((h + w) ns 0.01), line_width = round(fs / 10),
 *   font_size = fs (0: the Annotator's own fallbacks from the mosaic's size).  Per image i in order: a white outline of width 2 on
 *   [x, y, x + w, y + h] (x, y now in output pixels: w (i / ns), h (i % ns)); the file name Path(path).name[:40] in (220, 220, 220) at
 *   (x + 5, y + 5); then the image's boxes in their order through box_label in colors(cls).
 * Label mosaic: the image's labels carried into network pixels (the dataloader's xywhn2xyxy with the letterbox ratio and padding,
 *   xyxy2xywhn(clip, eps 1e-3), val.py's * (W, H, W, H)), then xywh2xyxy, * (w, h, w, h) if boxes.max() <= 1.01 else * scale when scale < 1,
 *   + (x, y); float32 in upstream's order; text names[cls].
 * Prediction mosaic: the image's NMS output in network pixels, the first 300 rows, xyxy2xywh then the same chain; only conf > 0.25 is
 *   drawn, text '{name} {conf:.1f}'; boxes are not clipped to their cell, primitives apply in index order.
 * File: Image.save(fname), Pillow's defaults: quality 75, 4:2:0, standard Huffman tables (aq_image_jpeg_coefs_q / aq_write_image_files_q at 75).
 *
 * aq_val_mosaic_u8 writes the (resized) mosaic in one launch; the source mosaic is never materialised.  batch_dev: n images of H x W x 3
 * one after the other; out_dev: out_h x out_w x 3 with out_h = ns h, out_w = ns w.  xtab / ytab: out_w / out_h entries (i0, i1, w0, w1) of
 * the ns W -> out_w and ns H -> out_h resizes, 11-bit weights as aq_letterbox_u8's (the identity tables when nothing is resized), in device
 * memory (16-byte aligned) and again in host memory, where every index is checked against [0, ns W) / [0, ns H).  Each tap resolves to
 * pixel (sx - W cx, sy - H cy) of image cx ns + cy, or to 255 when that is >= n.  Refused (AQ_ERR_INVALID, nothing written): null
 * pointers, n outside [1, 16], ns ns < n or ns > 4, non-positive sizes, an output that is not ns h x ns w, a table index outside the
 * source mosaic, buffers too small. */
int aq_val_mosaic_u8(const uint8_t* batch_dev, long long batch_bytes, int n, int ns, int H, int W, int h, int w, uint8_t* out_dev,
                     long long out_bytes, int out_h, int out_w, const int32_t* xtab_dev, const int32_t* xtab_host, const int32_t* ytab_dev,
                     const int32_t* ytab_host, void* stream);

/* --blank-key: what the reference's white-space key is made of (reference src/utils.py is_blank, is_partly_blank, the mask of
 * correct_partly_blank_geom), per w x h uint8 RGB image, in integers.  L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 (Pillow's convert("L"));
 * l_min, l_max = its extrema; blank_rows = rows whose 3 w bytes sum to >= 750 w, blank_cols = columns whose 3 h bytes sum to >= 750 h (an
 * average >= 250.); nonblank_px = pixels with max(R, G, B) < 250 and [x0, x1] x [y0, y1] their bounding box (inclusive; none: w, h, -1, -1). */
typedef struct aq_blank_stat { int32_t l_min, l_max, blank_rows, blank_cols, nonblank_px, x0, y0, x1, y1; } aq_blank_stat;
/* Frames are addressed as the frame encoder's (aq_frame; any base and pitch, w and h <= 65535, w h < 2^31); here mcu = the frame's first word
 * among the column sums of the scratch: the frames' columns follow each other from 0.  Scratch: 8 words per frame + one per column. */
size_t aq_blank_stats_scratch_bytes(const aq_frame* frames_host, int n_frames);
/* One read of every image on `stream`; the call initialises its scratch, allocates nothing and uses integer atomics only, so two calls give the
 * same bytes.  frames_host = frames_dev's content in host memory: a frame that leaves [images_dev, images_dev + image_bytes) is refused before
 * anything is launched.  n_frames = 0 does nothing. */
int aq_blank_stats_u8(const uint8_t* images_dev, long long image_bytes, const aq_frame* frames_dev, const aq_frame* frames_host, int n_frames,
                      void* scratch_dev, size_t scratch_bytes, aq_blank_stat* stats_dev, void* stream);

/* --blank-geom: the largest non-blank region of a partly blank tile (reference src/utils.py:482-530, correct_partly_blank_geom), in integers.
 * m = max(R, G, B) < 250.  Components: 8-connected on m; regions: 4-connected on ~m, every region that touches the frame's border being part
 * of one "outside" region.  A label is the row-major index y w + x of the first pixel (outside: -1).  An outer edge is a unit edge between a
 * pixel of m and the outside region or the frame's border; E(C) = sum over pixels (x, y) of C of (x + 1) [right neighbour outside] -
 * x [left neighbour outside] is the area inside C's exterior ring unless another component encloses C (then it is less than the encloser's).
 * The winner is arg max E, ties to the smallest label (the reference's tie order is rasterio's emission order, which is not pinned).
 * Record: examined (0: skipped, the rest as for no component); n_components; the winner's label (-1: none), pixel count, E, inclusive box
 * (none: w, h, -1, -1), outer edges and pixels with at least one outer edge. */
typedef struct aq_blank_geom { int32_t examined, n_components, label, px, area_px, x0, y0, x1, y1, n_edges, edge_px, reserved; } aq_blank_geom;
/* Frames as aq_blank_stats_u8 takes them (any base and pitch, w and h <= 65535, w h < 2^31 - 1); here mcu = the frame's first slot in the
 * scratch, a frame taking (w + 1) h + 2 slots rounded up to a multiple of 4, the frames' slots following each other from 0.  Scratch: 64
 * bytes per frame + 9 per slot (4 parent, 4 area accumulators, 1 mask), for every frame of the table, examined or not: 9.4 MB per 1024-px
 * tile, at most 2^31 slots per call.  A caller bounds it by examining the qualifying frames of a batch in groups. */
size_t aq_blank_geom_scratch_bytes(const aq_frame* frames_host, int n_frames);
/* Records of n_frames images of one buffer, on `stream`.  stats_dev (or null: every frame is examined) = the frames' aq_blank_stat records:
 * a frame is examined only if they say partly blank (not blank, blank_rows + blank_cols > 0) with nonblank_px > 0; the others are skipped on
 * the device.  labels_out_dev (or null): 2 int32 per slot, frame i's foreground map [h][w] at 2 mcu (label; -1 off the mask) and its
 * background map behind it (label; -1 outside region; -2 on the mask); examined frames only.  The same checks as aq_blank_stats_u8, before
 * anything is launched; the call initialises its scratch, allocates nothing and uses integer min / max / add atomics only, so two calls give
 * the same bytes.  n_frames = 0 does nothing. */
int aq_blank_components_u8(const uint8_t* images_dev, long long image_bytes, const aq_frame* frames_dev, const aq_frame* frames_host, int n_frames,
                           const aq_blank_stat* stats_dev, void* scratch_dev, size_t scratch_bytes, aq_blank_geom* records_dev,
                           int32_t* labels_out_dev, void* stream);
/* The winners' outer edges, from the scratch and the records aq_blank_components_u8 left for the same table: per winner pixel with an outer
 * edge two int32, (pixel index y w + x, side mask: 1 N, 2 E, 4 S, 8 W).  Frame i's go to pairs [edge_at[i], edge_at[i + 1]) of edges_dev (room
 * for edges_room pairs): edge_at = the running sum of the records' edge_px, given in device and in host memory.  The order inside a slice
 * depends on scheduling; the set does not. */
int aq_blank_ring_edges_u8(const aq_frame* frames_dev, const aq_frame* frames_host, int n_frames, const void* scratch_dev, size_t scratch_bytes,
                           const aq_blank_geom* records_dev, const long long* edge_at_dev, const long long* edge_at_host, int32_t* edges_dev,
                           long long edges_room, void* stream);

/* --facilities: DBSCAN of n points in metres, as sklearn.cluster.DBSCAN(eps, min_samples) labels them (reference src/cluster_facilities.py),
 * per dense group id: points of different groups never interact.  core = at least min_samples points of the group, the point itself
 * included, at dx dx + dy dy <= eps eps, evaluated in fp64 in exactly that form; a cluster = a connected component of core points; root =
 * the smallest original index among the cluster's core points; a point that is not core takes the smallest root among its core neighbours
 * and is noise (root -1) without one.  sklearn's label of a point is the rank of its root among the distinct roots of its group.
 * The points are addressed through a sort the caller made: key = group << 42 | cell_y << 21 | cell_x of a square grid whose cell edge is
 * above eps by enough that two points within eps never lie two cells apart, cell indices in [1, 2^21 - 2] (a free ring, so that the cells
 * cx - 1 .. cx + 1 of a row are one run of the sorted keys), group in [0, 2^21); keys_sorted_dev = the keys ascending, perm_dev = the original
 * index of every sorted position.  xy_dev ([n][2] doubles, 16-byte aligned) and group_dev stay in the caller's original order, as do the
 * outputs core_dev (uint8 [n]) and root_dev (int32 [n]). */
#define AQ_FACILITY_CELL_BITS 21
#define AQ_FACILITY_CELL_MASK ((1LL << AQ_FACILITY_CELL_BITS) - 1)
/* Scratch: 41 bytes per point (16 coordinates in sorted order, 24 key runs, 1 core flag), each array rounded up to 16 bytes; 0 for n <= 0 or
 * n >= 2^31. */
size_t aq_facility_scratch_bytes(long long n);
/* On `stream`; the call initialises its scratch, allocates nothing and uses integer min atomics only, so two calls give the same bytes.
 * n = 0 does nothing.  n >= 2^31, a null pointer, eps <= 0 (or not finite), min_samples < 1 and too little scratch are refused before
 * anything is launched.  An entry of perm_dev outside [0, n) is skipped on the device (its point stays unwritten); keys that are not
 * sorted or not those of the points, and a perm_dev that is no permutation, give wrong labels but no access outside the arrays. */
int aq_facility_dbscan_f64(const long long* keys_sorted_dev, const int32_t* perm_dev, const double* xy_dev, const int32_t* group_dev, long long n,
                           double eps, int min_samples, void* scratch_dev, size_t scratch_bytes, uint8_t* core_dev, int32_t* root_dev,
                           void* stream);

/* ---- --evaluate (evaluate.hip): the device steps of the cage-level precision / recall grid (reference src/get_kfold_cluster_performance.py) ----
 * aq_eval_member_conf_f64: for the points, sort and groups of aq_facility_dbscan_f64 and a confidence per point (conf_dev, [n] doubles, original
 * order), member_conf_dev[i][m - 1] (doubles [n][K], original order) = the largest confidence threshold c at which sklearn's DBSCAN(eps,
 * min_samples = m) over the points of confidence >= c gives point i a label >= 0: min(c_i, max over the points j within eps of i of
 * min(c_j, m-th largest confidence within eps of j)), -inf where no threshold does.  Every value is one of the inputs, bit for bit. */
/* Scratch: 48 + 8 K bytes per point (coordinates, key runs, confidences in sorted order and the core thresholds), each array rounded up to
 * 16 bytes; 0 for n <= 0, n >= 2^31 or K outside 1 .. 16. */
size_t aq_eval_scratch_bytes(long long n, int K);
/* On `stream`; the call initialises its scratch, allocates nothing and uses no atomics, so two calls give the same bytes.  n = 0 does nothing.
 * n >= 2^31, K outside 1 .. 16, a null pointer, eps <= 0 (or not finite), an unaligned array and too little scratch are refused before
 * anything is launched.  Keys and a perm_dev the caller got wrong give wrong values but no access outside the arrays (as above). */
int aq_eval_member_conf_f64(const long long* keys_sorted_dev, const int32_t* perm_dev, const double* xy_dev, const int32_t* group_dev,
                            const double* conf_dev, long long n, double eps, int K, void* scratch_dev, size_t scratch_bytes,
                            double* member_conf_dev, void* stream);
/* aq_box_match_f64: Q query boxes (qbox_dev [Q][4] doubles x0, y0, x1, y1, 32-byte aligned; qgroup_dev [Q]) against N key boxes (kbox_dev [N][4],
 * 32-byte aligned) sorted by (group, x0), group_start_dev [G + 1] = each group's first key, group_start_dev[G] = N.  hit_dev[q] (uint8) = 1 if
 * the closed box of query q intersects the closed box of a key of its group (touching edges and corners count), else 0; a group outside
 * [0, G) matches nothing.  With payload_dev ([N][K] doubles, K in 1 .. 16) out_dev[q][m] = the maximum of payload[k][m] over the matching
 * keys k, -inf when none match; without one (K = 0) neither pointer is used.  On `stream`, no atomics, one launch; Q = 0 does nothing.
 * Q or N >= 2^31, G < 0, K out of range, a null pointer and an unaligned array are refused before anything is launched; group starts are
 * kept inside [0, N] on the device. */
int aq_box_match_f64(const double* qbox_dev, const int32_t* qgroup_dev, long long Q, const double* kbox_dev, long long N,
                     const int32_t* group_start_dev, int G, const double* payload_dev, int K, uint8_t* hit_dev, double* out_dev, void* stream);

/* ---- --evaluate-kfold (eval_subsets.hip): the two steps above for up to 32 subsets of one point set in one call (the folds of the reference's
 * StratifiedKFold).  A subset is one bit of a uint32 word per point: point i belongs to subset s (0 <= s < S) iff bit s of its word is set;
 * bits at and above S are ignored.
 * aq_eval_member_conf_subsets_f64: the arguments of aq_eval_member_conf_f64 plus mask_dev ([n] uint32, original order) and S in 1 .. 32.
 * member_conf_dev (doubles [S][n][K]): row [s][i] = what aq_eval_member_conf_f64 gives point i when only the points of subset s exist, that is
 *   T_s(i, m) = min(c_i, m-th largest confidence among the points of s within eps of i)     (-inf: fewer than m)
 *   M_s(i, m) = min(c_i, max over the points j of s within eps of i of T_s(j, m))
 * for i in s; a row of a point outside s is -inf.  Every value is one of the inputs, bit for bit, or -inf. */
/* Scratch: 52 + 8 K S bytes per point (coordinates, key runs, confidences and mask words in sorted order, the core thresholds of every subset),
 * each array rounded up to 16 bytes; 0 for n <= 0, K outside 1 .. 16, S outside 1 .. 32, n >= 2^31 or S n K >= 2^36. */
size_t aq_eval_subsets_scratch_bytes(long long n, int K, int S);
/* On `stream`; one gather and one set of key runs for all subsets; the call initialises what it reads of its scratch, allocates nothing and
 * uses no atomics, so two calls give the same bytes.  n = 0 does nothing.  S outside 1 .. 32, K outside 1 .. 16, n >= 2^31, S n K >= 2^36,
 * eps <= 0 (or not finite), a null pointer, an unaligned array and too little scratch are refused before anything is launched.  Keys and a
 * perm_dev the caller got wrong give wrong values but no access outside the arrays; the rows of an entry of perm_dev outside [0, n) stay
 * unwritten. */
int aq_eval_member_conf_subsets_f64(const long long* keys_sorted_dev, const int32_t* perm_dev, const double* xy_dev, const int32_t* group_dev,
                                    const double* conf_dev, const uint32_t* mask_dev, long long n, double eps, int K, int S,
                                    void* scratch_dev, size_t scratch_bytes, double* member_conf_dev, void* stream);
/* aq_box_match_subsets_f64: the arguments of aq_box_match_f64 plus qmask_dev ([Q] uint32), kmask_dev ([N] uint32, in the keys' sorted order) and
 * S in 1 .. 32; payload_dev is [S][N][K] doubles (keys in sorted order) or null with K = 0.  hitmask_dev[q] (uint32) = qmask[q] & the OR of
 * kmask[k] over the keys k of q's group whose closed boxes meet q's (bits at and above S cleared): bit s says that q is in subset s and meets
 * a key of subset s.  With a payload, out_dev[s][q][m] (doubles [S][Q][K]) = the maximum of payload[s][k][m] over the matching keys k that have
 * bit s, -inf when there is none or when q is not in s.  On `stream`, no atomics, one launch, every output element written; Q = 0 does
 * nothing.  S or K out of range, Q or N >= 2^31, S Q K or S N K >= 2^36, G < 0, a null pointer and an unaligned array (boxes 32 bytes, doubles
 * 8, words 4) are refused before anything is launched; group starts are kept inside [0, N] on the device. */
/* Scratch of the join: none (0 bytes); (size_t)-1 for sizes the launcher refuses, so that a caller can ask before it allocates outputs. */
size_t aq_box_match_subsets_scratch_bytes(long long Q, long long N, int K, int S);
int aq_box_match_subsets_f64(const double* qbox_dev, const int32_t* qgroup_dev, const uint32_t* qmask_dev, long long Q, const double* kbox_dev,
                             const uint32_t* kmask_dev, long long N, const int32_t* group_start_dev, int G, const double* payload_dev, int K, int S,
                             uint32_t* hitmask_dev, double* out_dev, void* stream);

/* ---- --model-errors (model_errors.hip): the cage-area error distributions (reference src/utils_tonnage.py:130-203, :284-327) ----
 * aq_model_error_match_f64: the queries, sorted keys and group starts of aq_box_match_f64, with qarea_dev [Q] (the queries' areas), krow_dev [N]
 * (the original row number of each sorted key; rows are distinct and >= 0, a negative one is skipped) and karea_dev [N] (the keys' areas, in
 * sorted order).  A key is a candidate of a query when aq_box_match_f64 would count it; inter = (min(q.x1, k.x1) - max(q.x0, k.x0)) *
 * (min(q.y1, k.y1) - max(q.y0, k.y0)), two subtractions and one product.  The match is the candidate of the largest inter; among equal inter the
 * smallest row wins; a NaN inter loses to every number.  match_dev[q] (int32) = that key's row, -1 without a candidate; overlap_dev[q] = 100 *
 * inter / ((q.x1 - q.x0) * (q.y1 - q.y0)) (inf for a query without area); error_dev[q] = karea[match] - qarea[q]; both NaN without a candidate,
 * and every NaN written is 0x7FF8000000000000.  On `stream`, one wavefront per query, no atomics, one launch; Q = 0 does nothing.  Q or N >= 2^31,
 * G < 0, a null pointer (the three key arrays may be null when N = 0) and an unaligned array (boxes 32 bytes, doubles 8, int32 4) are refused
 * before anything is launched; group starts are kept inside [0, N] on the device. */
int aq_model_error_match_f64(const double* qbox_dev, const int32_t* qgroup_dev, const double* qarea_dev, long long Q, const double* kbox_dev,
                             const int32_t* krow_dev, const double* karea_dev, long long N, const int32_t* group_start_dev, int G,
                             int32_t* match_dev, double* overlap_dev, double* error_dev, void* stream);
/* aq_model_error_moments_f64: query q is a member of moment group g when match_dev[q] >= 0, mgroup_dev[q] == g and error_dev[q] is finite.  Per
 * group n_dev[g] (int64) = its members, mean_dev[g] = S / n, sd_dev[g] = sqrt(D / n) (the population sd, scipy.stats.norm.fit) with S = the sum
 * of error and D = the sum of (error - mean)^2 in one written order: lane l of 64 adds the rows q = l, l + 64, ... in increasing q, +0.0 for a
 * non-member; the 64 partials then fold as v[i] + v[i + 32], + 16, ... + 1.  n = 0: mean and sd are NaN (0x7FF8000000000000).  fp64 in + - x /
 * sqrt only, nothing contracted.  On `stream`, one wavefront per group, no atomics, one launch; G = 0 does nothing.  Q or G >= 2^31, a null
 * pointer (the three inputs may be null when Q = 0) and an unaligned array are refused before anything is launched. */
int aq_model_error_moments_f64(const double* error_dev, const int32_t* match_dev, const int32_t* mgroup_dev, long long Q, long long G,
                               long long* n_dev, double* mean_dev, double* sd_dev, void* stream);

/* --land-filter: which of N boxes (x0, y0, x1, y1; x0 <= x1, y0 <= y1) lie on land (reference src/process_yolo/geocode_results.py:200-218:
 * sjoin with the predicate `intersects`), against the E segments (ax, ay, bx, by) of all rings of the land polygons, exterior and holes
 * alike; everything fp64, EPSG:3857 metres.  One byte per box: bit 0 = some segment meets the closed box (the bounding boxes overlap, closed,
 * and the box's four corners are not all strictly on one side of the segment's line), bit 1 = the corner (x0, y0) is inside the land under
 * the even-odd rule (crossings of the ray towards +x, half-open in y: (ay <= y0) != (by <= y0), the corner strictly left of an upward
 * segment or strictly right of a downward one).  Both use the sign of orient(a, b, c) = (bx - ax) (cy - ay) - (by - ay) (cx - ax) in exactly
 * that form.  The box is on land when the byte is not 0; touching counts.
 * The segments are addressed through a band table the caller made: band(y) = floor((y - Y0) / h) clamped to [0, nbands), every segment
 * entered in each band from band(min y) to band(max y); entry_seg_dev = the entries' segment indices band by band, band_start_dev
 * [nbands + 1] = each band's first entry, band_start_dev[nbands] = entries.  A box wholly below Y0 or with floor((y0 - Y0) / h) >= nbands
 * gets 0: the table has to cover every segment without clamping (floor((max y - Y0) / h) < nbands), as engine.land_flags builds it. */
/* Scratch: 32 bytes per entry (the segments' coordinates in entry order); 0 for entries <= 0 or entries >= 2^31. */
size_t aq_land_scratch_bytes(long long entries);
/* On `stream`; the call initialises its scratch, allocates nothing and uses no atomics, so two calls give the same bytes.  N = 0 does nothing;
 * E = 0 (or entries = 0) zeroes flags_dev.  E, N or entries >= 2^31, h <= 0, h or Y0 not finite, nbands < 1, a null pointer, seg_dev, boxes_dev
 * or scratch_dev not 32-byte aligned and too little scratch are refused before anything is launched.  An entry outside [0, E) meets nothing
 * and band starts are kept inside [0, entries] on the device, so a table the caller got wrong gives wrong flags but no access outside the
 * arrays. */
int aq_land_filter_f64(const double* seg_dev, long long E, const int32_t* entry_seg_dev, long long entries, const int32_t* band_start_dev,
                       int nbands, double Y0, double h, const double* boxes_dev, long long N, void* scratch_dev, size_t scratch_bytes,
                       uint8_t* flags_dev, void* stream);

/* --land-images: which of N image rectangles (x0, y0, x1, y1; x0 <= x1, y0 <= y1) lie wholly on land, at least `indent` metres from the
 * coast (reference src/utils.py:46-69, mark_land_images: `within` the land shrunk by buffer(-5)), against the same segments through the same
 * band table as aq_land_filter_f64.  Per rectangle dist2_dev = the squared distance to the nearest land edge -- 0 for an edge that meets
 * the closed rectangle (the land filter's bit-0 predicate), else the minimum of the four corners' squared distances to the segment and the
 * two segment ends' to the rectangle, every expression as the head comment of csrc/land_images.hip writes it -- over the segments of the
 * bands floor((y0 - 3 indent - Y0) / h) .. floor((y1 + 3 indent - Y0) / h), capped at (2 indent)^2, so that it does not depend on the band
 * height; and one byte: bit 0 = dist2 < indent^2, bit 1 = the land filter's corner parity for (x0, y0).  The image is on land when the
 * byte is 2.  A rectangle wholly above or below all bands, or with a coordinate that is not a number, gets byte 0 and dist2 = (2 indent)^2. */
/* Scratch: 32 bytes per entry (the segments' coordinates in entry order); 0 for entries <= 0 or entries >= 2^31. */
size_t aq_land_images_scratch_bytes(long long entries);
/* On `stream`; the call initialises its scratch, allocates nothing and uses no atomics, so two calls give the same bytes.  N = 0 does nothing;
 * E = 0 (or entries = 0) gives byte 0 and dist2 = (2 indent)^2 everywhere.  Refused before anything is launched, both outputs untouched: what
 * aq_land_filter_f64 refuses, an indent that is not positive and finite, dist2_dev null or not 8-byte aligned. */
int aq_land_images_f64(const double* seg_dev, long long E, const int32_t* entry_seg_dev, long long entries, const int32_t* band_start_dev,
                       int nbands, double Y0, double h, const double* rects_dev, long long N, double indent, void* scratch_dev,
                       size_t scratch_bytes, uint8_t* flags_dev, double* dist2_dev, void* stream);

/* ---- --tonnage (tonnage.hip): the bootstrap of the facilities' live-weight production per image pass (reference src/utils_tonnage.py:28-127,
 * compute_facility_tonnage_estimates, with :330-458, sample_model_errors).  Everything fp64; the only floating-point operations are + - x /
 * sqrt, comparisons and selections (no fma, no libm), so aquaculture_amd.tonnage.simulate_numpy gives the same bytes.
 * Random numbers.  Philox4x32-10 (multipliers D2511F53, CD9E8D57; key increments 9E3779B9, BB67AE85), key = (seed & 0xffffffff, seed >> 32),
 * counter words (c0, c1, c2, c3) = (simulation k, entity, slot, attempt): a draw depends on nothing else.  Slots: 0 model error (entity = the
 * entry's index; attempt = 0, 1 ..), 1 area, 2 Bernoulli, 3 depth A, 4 depth B, 5 stocking, 6 harvest (entity = the facility's index,
 * attempt 0).  With output words w0 .. w3: x = ((w1 << 32) | w0) >> 11, u = ((double)x + 0.5) 2^-53, and 1 - 2^-53 where that rounds to 1.
 * alog(x), x > 0: x = m 2^e, 0.5 <= m < 1; m < 0.7071067811865476: m = 2 m, e = e - 1; s = (m - 1) / (m + 1), s2 = s s; acc = 1/27, then
 * acc = acc s2 + 1/j for j = 25, 23 .. 1; alog = e 0.6931471805599453 + (2 s) acc.
 * ndtri(p): the Cephes Math Library's rational approximations with alog for log: NaN outside [0, 1], -inf at 0, +inf at 1; y = p, or 1 - p when
 * p > 1 - e^-2; y > e^-2: y = y - 0.5, y2 = y y, (y + y ((y2 P0(y2)) / Q0(y2))) sqrt(2 pi); else x = sqrt(-2 alog(y)), x0 = x - alog(x) / x,
 * z = 1 / x, x1 = (z P(z)) / Q(z) with (P1, Q1) for x < 8 and (P2, Q2) from 8 on; x0 - x1 when y was mirrored, else x1 - x0 as -(x0 - x1).
 * Horner from the leading coefficient.
 * Facility f owns the entries entry_start[f] .. entry_start[f + 1] - 1 (a cage of a facility each): area_orig (entry_area_dev [E]), the
 * model error's (mean, sd) (entry_err_dev [E][2], 16-byte aligned) and flags (entry_flags_dev [E]): bits 0-1 the kind (0 full ellipse, 1
 * border ellipse, 2 square; 3 as 0), bit 2 in the min selection, bit 3 in the max selection, bit 4 in the random selection (carried, not
 * used: the reference's point estimate).  In simulation k, for the entries in ascending order:
 *   area = area_orig + (mean + sd ndtri(u(k, e, 0, attempt))), attempt = 0, 1 .. while area <= 0; after 64 such draws area = area_orig (the
 *   reference draws for ever); (min_c, max_c) = (area, area), ((4 area) / (2 + pi), ((2 pi) area) / (2 + pi)), ((2 area) / 3, (4 area) / 3)
 *   by kind; lo = lo + min_c with bit 2, hi = hi + max_c with bit 3, both from +0.
 * Then sim_area = lo + (hi - lo) u1; with d = depth_dev[f] and m = min_depth: depth = m unless d > m (the reference divides 0 by 0 at d = m),
 * else u2 < mix: d + ((d - m) / 1.96) ndtri(pA0 + u3 (pA1 - pA0)), otherwise d + (d / 1.96) ndtri(pB0 + u4 (pB1 - pB0)), depth_probs (host
 * memory) = pA0, pA1, pB0, pB1 = Phi(-1.96), Phi(0), Phi(0), Phi(1.96); with the six doubles of the facility's pass (pass_dev[f], kept inside
 * [0, P) for this) s_mean, s_sd, pS0, pS1, h_mean, h_sd: stocking = s_mean + s_sd ndtri(pS0 + u5 (pS1 - pS0)), harvest = h_mean + h_sd
 * ndtri(u6); ton_dev[(k - k0) F + f] = ((sim_area depth) stocking) (harvest (1 / 1000)).
 * On `stream`, one launch, allocates nothing, no atomics: the same bytes on every call, whatever k0 and K_chunk split the simulations into.
 * F = 0 or K_chunk = 0 does nothing.  Refused before anything is launched: K_chunk, F or E >= 2^31, K_chunk F >= 2^62, k0 < 0 or
 * k0 + K_chunk > 2^32, a null pointer, an unaligned array, mix outside [0, 1], a min_depth, depth probability or pass parameter that is not
 * finite, s_sd <= 0, P < 1, and offsets in entry_start_host (= entry_start_dev's content in host memory; pass_params_host likewise) that
 * decrease or leave [0, E].  On the device entry ranges are kept inside [0, E], so tables the caller got wrong give wrong numbers but no
 * access outside the arrays. */
int aq_tonnage_simulate_f64(unsigned long long seed, long long k0, long long K_chunk, const int32_t* entry_start_dev,
                            const int32_t* entry_start_host, long long F, const double* entry_area_dev, const double* entry_err_dev,
                            const uint8_t* entry_flags_dev, long long E, const double* depth_dev, const int32_t* pass_dev,
                            const double* pass_params_dev, const double* pass_params_host, int P, double mix, double min_depth,
                            const double* depth_probs, double* ton_dev, void* stream);
/* The sums over ton_dev [K_chunk][F], each a plain sequence of fp64 additions in the stated order:
 *   T_dev[k][p] ([K_chunk][P]) = the sum of ton[k][f] over the facilities with pass_dev[f] == p in ascending f, from +0 (a pass without
 *   facilities: +0; a pass id outside [0, P) enters no sum);
 *   moments_dev[f] ([F][2], 16-byte aligned, caller-held) = (moments[f][0] + sum, moments[f][1] + sum of squares) of ton[.][f], t and t t
 *   added one after the other in ascending k, so that the chunks of a run add up in one fixed order.
 * On `stream`, two launches, no atomics.  K_chunk = 0 does nothing; counts >= 2^31, a null pointer and an unaligned array are refused. */
int aq_tonnage_reduce_f64(const double* ton_dev, long long K_chunk, long long F, const int32_t* pass_dev, int P, double* T_dev,
                          double* moments_dev, void* stream);
/* Test hooks: out_dev[i] = ndtri(p_dev[i]); out_dev[i] = the uniform of counter counters_dev[i][0 .. 3] (uint32) under `seed`. */
int aq_tonnage_ndtri_f64(const double* p_dev, long long n, double* out_dev, void* stream);
int aq_tonnage_uniform_f64(unsigned long long seed, const uint32_t* counters_dev, long long n, double* out_dev, void* stream);

/* ---- --performance (population.hip): the samples behind the upper bound on the cage population (reference
 * src/Results/upper_bound_calculation.R: if a fraction r of a stratum's images held cages, how many positives would a sample of S of them
 * hold?).  For the simulations k0 <= k < k0 + K, on `stream`, one launch:
 *   counts_dev[k - k0][i] ([K][R] int32, caller-held) = #{j < S : u(k, j) < rates[i]}, the comparison in fp64,
 *   u(k, j) = the generator of --tonnage (Philox4x32-10, key = the low and the high word of `seed`) at counter (k, j >> 1, 16, 0): of its four
 *   words (w0, w1, w2, w3) an even j takes (w1 : w0) and an odd j (w3 : w2), through the same 53-bit rule ((x >> 11) + 0.5) 2^-53, capped
 *   below 1.  Slot 16 is none of the bootstrap's (0 .. 6).  Every rate is compared with the same uniforms, so a row never decreases where
 *   the rates increase.  performance.counts_numpy gives the same bytes.
 * rates_dev / rates_host = the R rates on the device and on the host (the same values; the host copy is the one that is checked).
 * Refused before any launch: R outside 1 .. 16, S outside 1 .. 2^31 - 1, K < 0, k0 < 0, k0 + K > 2^32 (k is one counter word), a rate
 * that is NaN or outside [0, 1], a null pointer.  K = 0 does nothing.  One wavefront per simulation, no atomics. */
int aq_bernoulli_counts_i32(unsigned long long seed, long long k0, long long K, long long S, const double* rates_dev, const double* rates_host,
                            int R, int32_t* counts_dev, void* stream);

/* ---- --bathymetry (depth.hip): min, max, sum and count of the depth raster's cells under every facility (reference
 * src/utils_tonnage.py:591-665, add_facility_depth: rasterstats.zonal_stats(all_touched=True) over the union of a facility's circle and square
 * cages).  raster_dev: float32 [nrows][ncols], row 0 the northernmost; cell (r, c) is the half-open square [x0 + c dx, x0 + (c + 1) dx) x
 * (y0 - (r + 1) dy, y0 - r dy].  Facility f owns the cages entry_start[f] .. entry_start[f + 1] - 1 of cages_dev [E][4] (lon_min, lon_max,
 * lat_min, lat_max; 32-byte aligned).  Only fp64 - / floor, comparisons and selections decide a cell, only fp64 + in one written order makes
 * the sum, so aquaculture_amd.bathymetry.stats_numpy gives the same bytes.
 * aq_depth_ranges_f64: c0 = floor((lon_min - x0) / dx), c1 = floor((lon_max - x0) / dx), r0 = floor((y0 - lat_max) / dy), r1 = floor((y0 -
 * lat_min) / dy), each kept inside [-1, ncols] / [-1, nrows] in fp64 before the conversion (what is not >= -1, NaN included, gives -1); the cage
 * touches columns c0 .. c1 and rows r0 .. r1 intersected with the raster's: cage_range_dev [E][4] int32 (c0, c1, r0, r1; 16-byte aligned),
 * (0, -1, 0, -1) for a cage without a cell or with a NaN coordinate.  window_dev [F][4] (16-byte aligned) = the bounding rectangle of the facility's cage ranges,
 * (0, -1, 0, -1) without any.  On `stream`, one launch, one wavefront per facility, no atomics.  F = 0 does nothing.  F or E >= 2^31, a negative
 * nrows or ncols, dx or dy not positive and finite, an origin that is not finite, a null pointer and an unaligned array are refused before
 * anything is launched; entry ranges are kept inside [0, E] on the device. */
int aq_depth_ranges_f64(const int32_t* entry_start_dev, long long F, const double* cages_dev, long long E, double x0, double y0, double dx,
                        double dy, int nrows, int ncols, int32_t* cage_range_dev, int32_t* window_dev, void* stream);
/* aq_depth_stats_f64: the facility's touched cells are the union of its cages' ranges, kept as bits of its own words of bitmap_dev
 * [bitmap_words] uint32, which the caller zeroed: with W the window's width, bit i (word i / 32, bit i % 32, from the facility's first word
 * word_start[f]) is cell (i / W, i % W) of the window, so facility f needs (cells + 31) / 32 words.  The bits are set with integer atomicOr.
 * Valid cells: touched, not NaN, not equal to nodata (a NaN nodata excludes nothing).  stats_dev [F][3] = min, max (the float32 values
 * widened; a zero is +0.0) and sum; count_dev [F] int64.  The sum: partial l = 0 .. 63 starts at +0.0 and adds the valid cells with
 * i % 64 == l in ascending i; the partials are added in order of l from +0.0.  No valid cell: +inf, -inf, +0.0, 0.
 * window_host and word_start_host = the content of window_dev and word_start_dev in host memory, checked there.  Refused before anything is
 * launched: F or E >= 2^31, bitmap_words >= 2^31, a window of 2^31 cells or more or one that leaves the raster, a facility with fewer words
 * than its window needs, word starts that decrease or leave [0, bitmap_words], a null pointer, an unaligned array.  On the device the
 * windows are kept inside the raster, the cage ranges inside the window, the entries inside [0, E], and a window that does not fit its
 * words counts as empty: tables the caller got wrong give wrong numbers but no access outside the arrays.  On `stream`, one launch, one
 * wavefront per facility, no floating-point atomics: the same bytes on every call.  F = 0 does nothing. */
int aq_depth_stats_f64(const int32_t* entry_start_dev, long long F, const int32_t* cage_range_dev, long long E, const int32_t* window_dev,
                       const int32_t* window_host, const long long* word_start_dev, const long long* word_start_host, const float* raster_dev,
                       int nrows, int ncols, double nodata, uint32_t* bitmap_dev, long long bitmap_words, double* stats_dev,
                       long long* count_dev, void* stream);

/* ---- --dedup-years (dedup.hip): one year's cages per tile and image pass (reference src/utils_tonnage.py:668-911,
 * dedup_cages_in_overlap_years_with_white_space).  The images of one (pass, tile key) group share a pixel grid of w x h pixels; each image
 * that takes part is a slot (at most AQ_DEDUP_MAX_SLOTS, in ascending year) with a mask: the whole frame (AQ_DEDUP_FULL) or a bitmap
 * (AQ_DEDUP_BITMAP) of h rows x ceil((w + 1) / 32) uint32 words, bit c % 32 of word c / 32 of row r = pixel (c, r).  Under an order of the
 * slots, slot i is allotted its mask minus the masks before it; a cage of slot i with the closed pixel box [xmin, xmax] x [ymin, ymax]
 * survives iff the box meets a pixel square of that region, i.e. iff the window columns max(xmin - 1, 0) .. min(xmax, w - 1), rows
 * max(ymin - 1, 0) .. min(ymax, h - 1) holds a pixel of it.  All three launchers run on `stream`, allocate nothing, use integer atomics only
 * (the same bytes on every call), keep every index inside its array on the device -- tables the caller got wrong give wrong numbers but no
 * access outside the arrays -- and refuse before anything is launched: a count (vertices, rings, bitmap words, groups, cages) >= 2^31, a
 * null pointer, an unaligned array, and what each lists below, checked on the *_host copies of the device tables.
 * Tables: group [G][16] int32 (64 bytes; 16-byte aligned) = n, w, h, 0, kind[5], first bitmap word[5], 0, 0; cage [C][8] int32 (16-byte
 * aligned) = group, slot, xmin, xmax, ymin, ymax, 0, 0. */
#define AQ_DEDUP_MAX_SLOTS 5
#define AQ_DEDUP_MAX_PERMS 120
#define AQ_DEDUP_ABSENT 0
#define AQ_DEDUP_FULL 1
#define AQ_DEDUP_BITMAP 2
#define AQ_DEDUP_SEL_MIN 4       /* the bits aquaculture_amd.tonnage gives the selections */
#define AQ_DEDUP_SEL_MAX 8
#define AQ_DEDUP_SEL_RANDOM 16
/* aq_dedup_fill_u32: ring r = the vertices ring_start[r] .. ring_start[r + 1] - 1 of ring_xy_dev [V][2] int32 (x, y pixel corners, 8-byte
 * aligned), a closed walk (first vertex repeated at the end); ring_frame [R][4] int32 (16-byte aligned) = first bitmap word, w, h, 0: every
 * ring has a bitmap of its own in bitmap_dev [bitmap_words], which the caller zeroed.  Launch 1, one lane per vertex: the segment to the
 * next vertex of the same ring, if vertical at 0 <= x <= w, toggles bit x of the rows min(y) .. max(y) - 1 inside the frame with atomicXor
 * (x = w lands in the row's extra column); other segments toggle nothing.  Launch 2, one lane per row: the inclusive prefix XOR of the
 * row's bits, so that pixel (c, r) is set iff an odd number of the ring's unit edges in row r lie at x <= c: the even-odd fill of the
 * ring.  R = 0 does nothing.  Also refused: ring_start that decreases or leaves [0, V], a frame side outside [1, 32768], a bitmap that does
 * not fit bitmap_words. */
int aq_dedup_fill_u32(const int32_t* ring_xy_dev, long long V, const int32_t* ring_start_dev, const int32_t* ring_start_host,
                      const int32_t* ring_frame_dev, const int32_t* ring_frame_host, long long R, uint32_t* bitmap_dev,
                      long long bitmap_words, void* stream);
/* aq_dedup_sets_u32: words_dev[e] for every cage e: bit S (S = a set of slots as a number, bit j = slot j) is set iff some pixel of the
 * cage's window lies in the masks of exactly the slots of S among the group's n, and S holds the cage's own slot.  0 for a group outside
 * [0, G), a slot outside [0, n), an AQ_DEDUP_ABSENT slot and an empty window.  One wavefront per cage: lanes stride over the (row, word
 * column) positions of the window.  C = 0 does nothing.  Also refused: a group with n outside [1, 5] (the longest image pass has five
 * years), a frame side outside [1, 32768], a kind that is none of the three, a slot's bitmap that does not fit bitmap_words. */
int aq_dedup_sets_u32(const int32_t* group_dev, const int32_t* group_host, long long G, const int32_t* cage_dev, long long C,
                      const uint32_t* bitmap_dev, long long bitmap_words, uint32_t* words_dev, void* stream);
/* aq_dedup_select_f64: group g owns the cages cage_start[g] .. cage_start[g + 1] - 1.  Order number q of the n! is the q-th of
 * itertools.permutations(range(n)); a cage of slot i survives an order iff its word has a set without any slot placed before i.
 * sums_dev [G][120]: entry q < n! = the areas (area_dev [C]; a NaN counts as 0) of the order's survivors, added one cage at a time in
 * ascending e from +0.0 (fp64 + only); entries from n! on are +0.0.  One ordered walk over the n! sums: max = the last order whose sum is
 * >= the running best, which starts at 0; min = the first whose sum is < the running best, which starts at +inf (the reference's
 * comparisons, :770-775); random = random_order_dev [G][5] int32, slot random_order[g][k] being the k-th (an entry that is no slot of the
 * group is skipped, a slot that is not named comes last).  chosen_dev [G][4] int32 (16-byte aligned) = the order numbers of min, max and
 * random and n!; -1 where no order qualified, and then no cage survives that selection.  sel_dev [C] uint8: for the cages of the G groups,
 * AQ_DEDUP_SEL_MIN | _MAX | _RANDOM of the selections they survive (other cages are not written).  One wavefront per group, lanes over
 * the orders.  G = 0 does nothing.  Also refused: n outside [1, 5], cage_start that decreases or leaves [0, C]. */
int aq_dedup_select_f64(const int32_t* group_dev, const int32_t* group_host, const int32_t* cage_start_dev, const int32_t* cage_start_host,
                        long long G, const int32_t* cage_dev, const uint32_t* words_dev, const double* area_dev, long long C,
                        const int32_t* random_order_dev, uint8_t* sel_dev, int32_t* chosen_dev, double* sums_dev, void* stream);

/* ---- --tonnage-missing / --tonnage-near-sites: does a closed box meet a union of image regions (csrc/coverage.hip) ----
 * The reference's modify_cage_list_using_geometry (src/utils_tonnage.py:1108-1136): cage.intersects(the union of a pass's image polygons).
 * Definitions:
 *   image region   an image takes part under the rule of aquaculture_amd.dedup.build_problem -- status `complete`, or `partly blank` with a
 *                  ring in the blank-geom file -- if its name parses to a bbox_ind the wanted-bboxes table lists.  Its rectangle is
 *                  blank_geom.tile_bounds(name, wanted) = (west, south, east, north), EPSG:3857, fp64.  Complete image: the closed
 *                  rectangle.  Partly blank image: the closed even-odd region of the ring blank_geom.to_bounds(ring_px, west, south, east,
 *                  north), the vertices computed on the host in numpy by that expression, so both ends of a vertical segment hold the same
 *                  double; the kernel receives metres and only compares.
 *   coverage of p  the union of the regions of the images whose year maps to pass p; it does not depend on the de-duplication order.
 *   meets(B, i)    for a closed box B = (x0, y0, x1, y1).  Rectangle image: x0 <= east && x1 >= west && y0 <= north && y1 >= south.
 *                  Ring image: its rectangle meets B and (some segment's closed bounding box overlaps B -- the segments are axis-parallel,
 *                  so the segment meets B -- or an odd number of segments have (ay <= y0) != (by <= y0) && ax > x0: the corner (x0, y0)
 *                  strictly inside; the parity only decides when no segment meets B).  A box with a NaN meets nothing.
 *   first[q]       for query q = (box, target pass): the smallest image number of that pass whose region meets the box, or -1.  Images
 *                  are numbered in the host's order, sorted by (pass, image name).  Covered: first >= 0.
 * Everything is comparisons and integer minima: aquaculture_amd.missing.first_numpy gives the same bytes, and so do two launches.
 * Arrays: rect_dev [I][4] fp64 (32-byte aligned); ring_start [I + 1] int32, image i a ring image iff ring_start[i + 1] > ring_start[i], its
 * closed walk (first vertex repeated at the end) xy_dev [ring_start[i] .. ring_start[i + 1])[2] fp64 (16-byte aligned); band [P][2] fp64 =
 * Y0, h of every pass: band(y) = floor((y - Y0) / h) clamped to [0, nbands), image i of pass p entered in every band from band(south) to
 * band(north) by the same expression; entry_img_dev [entries] int32 lists the entries pass by pass and band by band, band_start
 * [P nbands + 1] int32 their first entries; box_dev [Q][4] fp64 (32-byte aligned), qpass_dev [Q] int32 (a pass outside [0, P): -1);
 * scratch_dev: 32 bytes per entry (32-byte aligned); first_dev [Q] int32, the only memory written beside the scratch.  Two launches on
 * `stream` (gather the rectangles into entry order; one wavefront per query), no atomics, plain vector stores.  Q = 0 does nothing; no
 * image, pass or entry: every first is -1.  Refused before anything is launched, by the arguments and the *_host copies alone: a negative
 * count or one >= 2^31 (ring vertices included: the starts are 32-bit), nbands < 1 or P nbands + 1 >= 2^31, ring starts or band starts that
 * are not sorted or leave [0, V] / [0, entries], a band height that is not positive and finite or a Y0 that is not finite, a null pointer,
 * an unaligned array, too little scratch. */
int aq_coverage_first_i32(const double* rect_dev, const int32_t* ring_start_dev, const int32_t* ring_start_host, long long I,
                          const double* xy_dev, long long V, const int32_t* entry_img_dev, long long entries,
                          const int32_t* band_start_dev, const int32_t* band_start_host, const double* band_dev, const double* band_host,
                          long long P, long long nbands, const double* box_dev, const int32_t* qpass_dev, long long Q, void* scratch_dev,
                          size_t scratch_bytes, int32_t* first_dev, void* stream);

/* ---- --dedup-overlaps: every cage once where the download boxes overlap (csrc/overlaps.hip) ----
 * The reference's deduplicate_download_boxes / deduplicate_gdf_with_bboxes (src/utils.py:241-322) for closed axis-parallel boxes
 * R_i = (x0, y0, x1, y1), fp64 EPSG:3857, in file order: a box yields to every box before it.  Definitions (DESIGN.md section 24;
 * aquaculture_amd.overlaps restates them in numpy and in plain loops), comparisons only:
 *   C_i          the earlier boxes j < i whose open interiors meet R_i's: x0_j < x1_i && x1_j > x0_i, likewise in y.
 *   grid         of box i over some boxes of C_i: xs = the distinct values of x0_i, x1_i and of those boxes' x0_j, x1_j clamped into
 *                [x0_i, x1_i], ys likewise; cell [xs[a], xs[a+1]] x [ys[b], ys[b+1]] is covered iff one of the boxes contains it.
 *   detection D  of box i, on the grid over P(D) = the boxes of C_i that meet the closed D.  state 0 (dropped): no uncovered cell meets
 *                the closed D; 1 (whole): uncovered cells and no covered one meet D's open interior; 2 (clipped): both kinds do;
 *                3 (touching): an uncovered cell meets the closed D, none its open interior.  For states 1 - 3, over the pieces cell ^ D
 *                of the uncovered cells that meet the closed D: clip_bounds = (min x0, min y0, max x1, max y1), clip_area = the sum of
 *                (x1 - x0) * (y1 - y0), added per grid row (left to right, from 0) and the row sums bottom to top.  State 0: NaN, area 0.
 *   has_region   of box i: D = R_i is not dropped (the box keeps a region of its own).
 *
 * aq_overlap_partners_f64: the lists C_i through horizontal bands: band(y) = floor((y - Y0) / h) clamped to [0, nbands); the host entered
 * box j in every band from band(y0_j) to band(y1_j) by the same expression; entry_box_dev [entries] int32 lists the entries band by band,
 * ascending inside a band, band_start_dev [nbands + 1] int32 the bands' first entries.  Two calls on the same tables.  partner_dev null:
 * the count pass and an exclusive scan -- start_dev [n + 1] int64 (8-byte aligned) receives the lists' first entries, start[n] their
 * total.  partner_dev [partner_cap] int32 given: the fill pass -- box i's partners at partner[start[i] .. start[i + 1]), ascending;
 * nothing beyond partner_cap entries is written.  One wavefront per box.  boxes_dev [n][4] fp64 (32-byte aligned).  n = 0: start[0] = 0.
 *
 * aq_overlap_clip_f64: det_row_dev [m] int32 = the box of every detection (a row outside [0, n) is dropped), dets_dev [m][4] fp64 (32-byte
 * aligned); state_dev [m] uint8, bounds_dev [m][4] fp64, area_dev [m] fp64, has_region_dev [n] uint8: the only memory written.  One
 * wavefront per detection, lanes over the partners, 64 at a time: no partner count and no grid is too large.  List entries outside [0, n)
 * and starts outside [0, T] are kept out on the device.  n = 0 and m = 0 does nothing.
 * Both: no atomics, plain vector stores, the caller's stream; two calls give the same bytes.  Refused before anything is launched: a count
 * outside [0, 2^31), nbands outside [1, 2^31 - 2], a band height that is not positive and finite, a Y0 that is not finite, a null pointer,
 * an unaligned array. */
int aq_overlap_partners_f64(const double* boxes_dev, long long n, const int32_t* entry_box_dev, long long entries,
                            const int32_t* band_start_dev, long long nbands, double Y0, double h, long long* start_dev,
                            int32_t* partner_dev, long long partner_cap, void* stream);
int aq_overlap_clip_f64(const double* boxes_dev, long long n, const long long* start_dev, const int32_t* partner_dev, long long T,
                        const int32_t* det_row_dev, const double* dets_dev, long long m, uint8_t* state_dev, double* bounds_dev,
                        double* area_dev, uint8_t* has_region_dev, void* stream);

/* ---- --facility-sites: which facilities lie at a site the literature knew, which are additional (csrc/facility_sites.hip) ----
 * The data behind the reference's map of known and additional production locations (src/Results/FacilitiesMaps.py: get_true_facilities
 * :64-94, classify_our_facilities :117-188, count_unique_locations :97-114).  All boxes are closed, (x0, y0, x1, y1), fp64, EPSG:3857;
 * meet(a, b) = a.x0 <= b.x1 && b.x0 <= a.x1 && a.y0 <= b.y1 && b.y0 <= a.y1: touching counts, a NaN meets nothing.  Definitions (DESIGN.md
 * section 25; aquaculture_amd.facility_sites restates them in numpy and in plain loops):
 *   bounds[f]      the minimum of xmin_3857 and ymin_3857 and the maximum of xmax_3857 and ymax_3857 over the facility's cage_ids of class
 *                  circle or square (rectangle cages do not enter), by selections v < m ? v : m from +inf and v > m ? v : m from -inf, so
 *                  a NaN coordinate is never selected.  No such cage, or a selection that is not finite: four NaNs, state no_bounds.
 *   pass           the facility's pass column, or image_pass(year).  EARLY = 2000-2004, 2005-2009, 2010-2012; LATE = 2013-2015,
 *                  2016-2018, 2019-2021; any other: state no_period.
 *   true           (with a truth file only) label_hits[f] = the circle and square labels whose year's pass is f's pass and whose box
 *                  bounds[f] meets; first_label[f] = the smallest such label row, -1 without; label_hits = 0: state not_true.
 *   sites          the rows of the site file grouped by distinct (lat, lon) ascending, num_cages summed; those whose EPSG:3857 point lies
 *                  inside the closed total bounds of the wanted-bboxes table, numbered in that order (site_index); the site box is
 *                  (x - 1000, y - 1000, x + 1000, y + 1000) in EPSG:3857.  site_hits[f], first_site[f]: as above, one group.
 *   type           early pass: site_hits = 0 additional, else known_early; late pass: site_hits > 0 known, else additional.
 *   unique         per period, over its additional facilities: N(i) = the j of the set whose bounds meet bounds[i] (i is in N(i)); in
 *                  ascending facility_index an unmarked i is unique and marks N(i); location[i] = i if unique, else the smallest unique
 *                  g < i with i in N(g).  The walk is sequential and runs on the host over the lists the device wrote.
 * Three launchers.  Each runs on `stream`, one launch, one wavefront per facility or query, no atomics, plain vector stores, no allocation;
 * comparisons, selections, integer adds and minima only, so two calls give the same bytes and the numpy restatements (bounds_numpy,
 * join_count_numpy, join_list_numpy) give them too.  Refused before anything is launched, by the arguments and the *_host copies alone:
 * a count that is negative or >= 2^31, starts or offsets that decrease or leave their array, a null pointer, an unaligned array.  On the
 * device every start and offset is kept inside its array all the same: tables the caller got wrong give wrong numbers but no access
 * outside the arrays.
 *
 * aq_facility_bounds_f64: facility f owns the entries entry_start[f] .. entry_start[f + 1] - 1 (int32 [F + 1], the CSR layout of
 * aq_depth_ranges_f64) of entry_box_dev [E][4] fp64 (32-byte aligned); entry_use_dev [E] uint8: 0 = the entry does not take part.  Lane l of
 * 64 walks the entries start + l, start + l + 64, ... in ascending order under the selections above; the 64 partials fold by halves,
 * m[i] = m[i + 32] < m[i] ? m[i + 32] : m[i] (> for the maxima), then 16, ... 1.  bounds_dev [F][4] fp64 (32-byte aligned), the only
 * memory written; every NaN is the canonical quiet NaN.  F = 0 does nothing. */
int aq_facility_bounds_f64(const int32_t* entry_start_dev, const int32_t* entry_start_host, long long F, const double* entry_box_dev,
                           const uint8_t* entry_use_dev, long long E, double* bounds_dev, void* stream);
/* aq_box_join_count_i32: qbox_dev [Q][4], qgroup_dev [Q] int32, kbox_dev [N][4] sorted by (group, x0) with group_start [G + 1] int32 -- the
 * queries, sorted keys and group starts of aq_box_match_f64 -- and kid_dev [N] int32, the original row of every sorted key.  count_dev [Q]
 * int32 = the number of keys of the query's group that meet it (the run is cut at key.x0 <= query.x1 by a binary search, the lanes stride
 * over the rest); first_dev [Q] int32 = the smallest kid among them, -1 when count is 0.  A group outside [0, G) and a NaN query: 0, -1.
 * Q = 0 does nothing; N = 0: every count is 0. */
int aq_box_join_count_i32(const double* qbox_dev, const int32_t* qgroup_dev, long long Q, const double* kbox_dev, const int32_t* kid_dev,
                          const int32_t* group_start_dev, const int32_t* group_start_host, long long N, long long G, int32_t* count_dev,
                          int32_t* first_dev, void* stream);
/* aq_box_join_list_i32: the same join; the kid of every meeting key, in ascending position of the sorted run, goes to
 * list_dev[offset[q] .. offset[q + 1]) (int32 [total]); offset [Q + 1] int64 (8-byte aligned) = the exclusive scan of
 * aq_box_join_count_i32's counts, made by the caller.  Per chunk of 64 keys: a ballot of the lanes whose key meets the query, lane l's
 * slot = running base + the number of set ballot bits below l, base += the ballot's popcount (uniform over the wavefront).  A slot at or
 * beyond offset[q + 1] is not written, so a query writes inside its own slice whatever the offsets say, and the slice of a query without a
 * match is left as it was.  Q = 0 does nothing. */
int aq_box_join_list_i32(const double* qbox_dev, const int32_t* qgroup_dev, long long Q, const double* kbox_dev, const int32_t* kid_dev,
                         const int32_t* group_start_dev, const int32_t* group_start_host, long long N, long long G,
                         const long long* offset_dev, const long long* offset_host, int32_t* list_dev, long long total, void* stream);

/* ---- yolov5/val.py: mAP against YOLO labels (csrc/val.hip) ----
 * Upstream's second entry point on trained weights [UPSTREAM val.py run(), process_batch; utils/metrics.py ap_per_class, compute_ap, box_iou;
 * utils/general.py non_max_suppression(multi_label=True)].  Every launcher runs on `stream`, allocates nothing and stores with plain vector
 * stores; products, sums and quotients are rounded once each, as written (no fma), so aquaculture_amd.val's numpy restatements
 * (expand_rows_numpy, match_numpy, confusion_numpy, scores_numpy) give the same bytes.  Refused before anything is launched: a count outside its range, a
 * null pointer, an unaligned array, starts or runs that decrease or leave their array, a scratch that is too small.
 *
 * aq_val_expand_rows_f32: pred_dev [B][N][5 + nc] (what aq_engine_forward_raw writes) -> rows_dev [B][M][5 + nc] for aq_nms_opts in full-rows
 * mode: one row per (source row r, class j) with obj > conf_thres and obj * cls_j > conf_thres (one fp32 product), in ascending (r, j),
 * carrying the source row's box and obj, cls_j in column 5 + j and zeros in the other class columns.  count_dev [B] = the rows emitted per
 * image, whatever M is.  Rows count[b] .. M - 1 get obj = 0 and no other store.  If any image emits more than M rows, rows_dev is not
 * written at all.  1 <= M <= N * nc < 2^31, B <= 65535.  scratch_dev: aq_val_expand_scratch_bytes(B, N, nc), 4-byte aligned. */
size_t aq_val_expand_scratch_bytes(int B, int N, int nc);
int aq_val_expand_rows_f32(const float* pred_dev, int B, int N, int nc, float conf_thres, int M, void* scratch_dev, size_t scratch_bytes,
                           float* rows_dev, int32_t* count_dev, void* stream);
/* aq_val_match: dets_dev [B][max_det] and counts_dev [B] as aq_nms_opts wrote them (network pixels, descending confidence; a count is read
 * as min(max(count, 0), max_det)); image b's labels are label_start[b] .. label_start[b + 1] - 1 (int32 [B + 1]) of label_box_dev [L][4]
 * fp32 (x1, y1, x2, y2 in original pixels, 16-byte aligned) and label_cls_dev [L] int32; geom_dev [B][5] fp32 = (pad x, pad y, gain, w0,
 * h0).  Per detection: v = (v - pad) / gain, clipped to [0, w0] or [0, h0] (scale_boxes, no rounding); iou = inter / (area_label + area_det
 * - inter + 1e-7) with inter = clamp(min(x2) - max(x1), 0) * clamp(min(y2) - max(y1), 0), all fp32 in that order; its best label is the
 * label of its class with the largest iou, the higher index among equal ones; bit i of its word is set iff iou >= iouv_host[i] and no
 * detection of lower index has the same best label and reaches iouv_host[i] (i < 10).  Image b's detection d goes to position
 * total_dev[0] + sum of the counts of the images before b + d of conf_out_dev (fp32), cls_out_dev (int32) and bits_out_dev (uint16), when that
 * position is below cap; a second launch adds the batch's detections to total_dev[0] (int64, 8-byte aligned).  scratch_dev: 10 L int32.
 * One wavefront per image.  B = 0 does nothing. */
int aq_val_match(const aq_det* dets_dev, const int32_t* counts_dev, int B, int max_det, const float* label_box_dev,
                 const int32_t* label_cls_dev, const int32_t* label_start_dev, const int32_t* label_start_host, long long L,
                 const float* geom_dev, const float* iouv_host, int32_t* scratch_dev, float* conf_out_dev, int32_t* cls_out_dev,
                 uint16_t* bits_out_dev, long long cap, long long* total_dev, void* stream);
/* aq_val_confusion: upstream's class confusion matrix [UPSTREAM utils/metrics.py ConfusionMatrix.process_batch, as val.py calls it: per
 * image, only for images with labels] on aq_val_match's inputs -- dets_dev, counts_dev, label_box_dev, label_cls_dev, label_start (device
 * and host), geom_dev as there, the same scale_boxes step and the same fp32 iou.  Per image: (1) a detection takes part iff its conf >
 * conf (fp32, strict); its best label is the label of ANY class with the largest iou among those with iou > iou (strict), the higher label
 * index among equal ious; it may have none.  (2) a label keeps, of the detections whose best label it is, the one with the largest iou,
 * the higher detection index among equal ones, and adds 1 to matrix[class of that detection][class of the label]; a label that keeps none
 * adds 1 to matrix[nc][its class]; a detection that loses its best label does not fall back to another.  (3) if the image has at least one
 * kept pair, every detection that takes part and that no label keeps adds 1 to matrix[its class][nc]; in an image without a kept pair the
 * detections add nothing (upstream's `if n:`).  (4) an image without labels adds nothing.  matrix_dev: int64 [(nc + 1)][(nc + 1)],
 * [predicted][true], index nc = background, 8-byte aligned; it is ADDED TO with integer atomics (zero it before the first call; one buffer
 * serves a sweep).  image_dev: int32 [B][4] = labels of the image, detections that take part, kept pairs, kept pairs of equal classes.
 * An image that holds a class outside [0, nc) -- any detection below its count, any label -- adds nothing to the matrix, gets (labels, 0,
 * 0, 0) and stores 1 into flag_dev[0] (int32; never cleared here: zero it once, read it after the sweep).  label_cls_host: the host copy
 * of label_cls_dev or NULL; when given, a label class outside [0, nc) is refused.  Also refused, before anything is launched and with
 * every output untouched: nc < 1, conf or iou not finite, iou <= 0.  scratch_dev: aq_val_confusion_scratch_bytes(B, max_det, L) = 8 L +
 * 4 B max_det (rounded up to 8) bytes, 8-byte aligned: the labels' keys (iou bits << 32 | detection; in LDS up to 512 labels per image),
 * the detections' best labels.  One wavefront per image, one launch.  B = 0 does nothing. */
size_t aq_val_confusion_scratch_bytes(int B, int max_det, long long L);
int aq_val_confusion(const aq_det* dets_dev, const int32_t* counts_dev, int B, int max_det, const float* label_box_dev,
                     const int32_t* label_cls_dev, const int32_t* label_cls_host, const int32_t* label_start_dev,
                     const int32_t* label_start_host, long long L, const float* geom_dev, int nc, float conf, float iou,
                     void* scratch_dev, size_t scratch_bytes, long long* matrix_dev, int32_t* image_dev, int32_t* flag_dev, void* stream);
/* aq_val_scores_f64: bits_dev [n] uint16 and conf_dev [n] fp32 sorted by (class ascending, confidence descending, detection index
 * ascending); run c of C (one per class that has labels, ascending) is the elements run_range[c][0] .. run_range[c][1] - 1 (int64 [C][2]),
 * n_l_dev [C] int32 its number of labels, run_chunk0 [C + 1] int32 the exclusive scan of ceil(run length / aq_val_score_chunk()).  With
 * tpc_k the inclusive integer sum of bit j over the run, recall_k = tpc_k / (n_l + 1e-16), precision_k = tpc_k / (k + 1) in fp64:
 * ap_dev [C][10] = the trapezoid sum, added in ascending x one term (x[k + 1] - x[k]) * (y[k + 1] + y[k]) / 2 at a time, of y = interp(x,
 * [0, recall.., 1], [1, precision.., 0] under its running maximum from the right) on x_dev [nx] (nx <= 128); for threshold 0, on px_dev
 * [npx]: r_dev [C][npx] = interp(-px, -conf, recall, left = 0), p_dev = interp(-px, -conf, precision, left = 1), pr_dev = interp(px, mrec,
 * mpre).  interp is np.interp's rule: j = the last index with xp[j] <= x; fp[j] when j is the last index or xp[j] == x, else
 * (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j]) * (x - xp[j]) + fp[j].  An empty run gives zeros throughout.  scratch_dev:
 * aq_val_scores_scratch_bytes(n, run_chunk0[C]) = 120 bytes per detection + 240 per chunk, 8-byte aligned.  C = 0 does nothing. */
int aq_val_score_chunk(void);
size_t aq_val_scores_scratch_bytes(long long n, long long nchunks);
int aq_val_scores_f64(const uint16_t* bits_dev, const float* conf_dev, long long n, const long long* run_range_dev,
                      const long long* run_range_host, const int32_t* n_l_dev, const int32_t* run_chunk0_dev,
                      const int32_t* run_chunk0_host, int C, const double* x_dev, int nx, const double* px_dev, int npx,
                      void* scratch_dev, size_t scratch_bytes, double* ap_dev, double* p_dev, double* r_dev, double* pr_dev,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AQ_ENGINE_H */
