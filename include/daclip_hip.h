/*
 * daclip_hip.h — C ABI of libdaclip_hip.so, the MI355X-native DA-CLIP + IR-SDE hot path.
 *
 * The reference (yeeecheng/DA-CLIP) has no native plugin API; its plug points are Python
 * callables. Each entry point below replaces one of them:
 *
 *   dac_create / dac_set_weight / dac_finalize_weights
 *       replace module construction + strict `load_state_dict`:
 *       open_clip/factory.py:99-106 (load_checkpoint), factory.py:365-404
 *       (create_model_from_pretrained), config/daclip-sde/models/base_model.py:92-105
 *       (load_network) and networks.py:10-15 (define_G -> ConditionalUNet(**setting)).
 *   dac_encode_image
 *       replaces DaCLIP.encode_image(image, control=True)   (open_clip/daclip_model.py:46-53)
 *       and, with degra_ctx NULL, encode_image(image, control=False) (daclip_model.py:54-55)
 *   dac_encode_text / dac_degradation_probs
 *       replace DaCLIP.encode_text (daclip_model.py:125-126 -> model.py:237-249) and the
 *       degradation-class scoring softmax(100 d^ t^T) -> argmax (evaluate_daclip.py:45-84)
 *   dac_unet_forward
 *       replaces the `sde.set_model(model)` callable: model(x, mu, t, text_context=,
 *       image_context=) -> noise (utils/sde_utils.py:163-164, 195-202;
 *       DenoisingUNet_arch.py:118-174)
 *   dac_sde_schedule
 *       replaces IRSDE._initialize                          (utils/sde_utils.py:84-154)
 *   dac_sde_reverse
 *       replaces IRSDE.reverse_posterior / reverse_sde      (utils/sde_utils.py:261-313)
 *       as one hipGraph-captured loop
 *   dac_posterior_step
 *       replaces IRSDE.reverse_posterior_step / reverse_sde_step (sde_utils.py:44-45, 227-231)
 *
 * Conventions: every tensor argument is a caller-owned DEVICE pointer to contiguous fp32
 * NCHW data (torch `data_ptr()`), on the handle's device. `stream` is a hipStream_t (NULL =
 * default stream). Functions return 0 on success and a negative DAC_E* code on error; the
 * message is available from dac_last_error(). A handle owns its weights, workspace and
 * graphs; calls on one handle must be serialised; handles on different devices are
 * independent (one handle per GPU / rank).
 */
#ifndef DACLIP_HIP_H
#define DACLIP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dac_handle dac_handle;

/* compute/storage dtype. DAC_FP8 (BASELINE configs[4]): bf16 activations and kernels, with
 * the block-scaled fp8 MFMA where its operands arrive as OCP e4m3 without VALU work: the UNet's
 * 64 -> 64 ResBlock block2 convs read the e4m3 tensor (one E8M0 exponent per pixel and 32
 * channels) that block1's epilogue writes, with e4m3 weights (one exponent per output channel,
 * tap and 32 input channels); the ViT's GEMMs take e4m3 weights (one exponent per 64 k).
 * DAC_F16: IEEE half weights and activations on the f16 MFMA, fp32 accumulate — the same
 * bytes and MFMA rate as DAC_BF16 with an 11-bit instead of 8-bit significand. */
enum dac_dtype { DAC_F32 = 0, DAC_BF16 = 1, DAC_FP8 = 2, DAC_F16 = 3 };
enum dac_src_dtype { DAC_SRC_F32 = 0, DAC_SRC_F16 = 1, DAC_SRC_BF16 = 2 };
enum dac_mode { DAC_POSTERIOR = 0, DAC_SDE = 1 };       /* DenoisingModel.test(mode=) */
enum dac_schedule { DAC_COSINE = 0, DAC_LINEAR = 1, DAC_CONSTANT = 2 };

enum dac_err {
  DAC_OK = 0,
  DAC_E_ARG = -1,        /* bad argument / shape / dtype */
  DAC_E_KEY = -2,        /* unknown state_dict key or shape mismatch */
  DAC_E_MISSING = -3,    /* dac_finalize_weights: required key never set (strict load) */
  DAC_E_STATE = -4,      /* call order (e.g. forward before finalize) */
  DAC_E_HIP = -5,        /* HIP runtime error */
  DAC_E_NOMEM = -6
};

/* Network configuration. UNet fields mirror options/test.yml network_G.setting
 * (DenoisingUNet_arch.py:22-23); vision fields mirror CLIPVisionCfg
 * (open_clip/model_configs/daclip_ViT-B-32.json). Zero `unet`/`vit` skips that network. */
typedef struct dac_config {
  int unet;
  int in_nc, out_nc, nf, depth, ch_mult[8], context_dim;
  int use_degra_context, use_image_context;
  int vit;
  int image_size, patch_size, width, layers, head_width, mlp_width, embed_dim;
  /* Text tower (CLIPTextCfg, open_clip/model_configs/daclip_ViT-B-32.json text_cfg); needs vit.
   * Zero `text` leaves it out (its checkpoint keys are then accepted and ignored). */
  int text;
  int context_length, vocab_size, text_width, text_heads, text_layers;
  /* Wild-IR UNet variant (config/wild-ir/models/modules/DenoisingUNet_arch.py:22-40):
   * unet_scale_half = 1 for `scale: 0.5` (extra Downsample/Upsample around the levels);
   * unet_st_from = first level with a SpatialTransformer (0 = 3, the daclip-sde rule). */
  int unet_scale_half, unet_st_from;
} dac_config;

int dac_create(int device, int dtype, const dac_config* cfg, dac_handle** out);
void dac_destroy(dac_handle* h);

/* Copy one reference state_dict tensor (host or device pointer) into the handle,
 * repacking it to the kernel layout. Keys use the reference names, e.g.
 * "downs.0.0.block1.proj.weight", "clip.visual.transformer.resblocks.0.attn.in_proj_weight",
 * "visual_control.transformer.zero_modules.0.weight". Keys the hot path does not use
 * (text tower, logit_scale) are accepted and ignored (returns 1). */
int dac_set_weight(dac_handle* h, const char* key, const void* data, const int64_t* shape,
                   int ndim, int src_dtype);
/* Strict check: every key the configured networks need was set. */
int dac_finalize_weights(dac_handle* h);

/* img [B,3,S,S] (preprocessed, S = image_size) -> image_ctx [B,E], degra_ctx [B,E] fp32.
 * degra_ctx NULL runs DaCLIP.encode_image(image, control=False) instead
 * (open_clip/daclip_model.py:54-55 -> CLIP.encode_image, model.py:233-235): the clip tower
 * alone, no controller hiddens, its features in image_ctx. */
int dac_encode_image(dac_handle* h, const float* img, int B, float* image_ctx,
                     float* degra_ctx, void* stream);

/* Text features (CLIP.encode_text, open_clip/model.py:237-249, via DaCLIP.encode_text
 * daclip_model.py:125-126): tokens [N, context_length] int64 device ids (open_clip.tokenize
 * output) -> text_features [N, embed_dim] fp32, unnormalised. Ids outside the vocabulary give
 * NaN features (never an out-of-bounds read). */
int dac_encode_text(dac_handle* h, const int64_t* tokens, int N, float* text_features, void* stream);

/* Degradation-class scoring (evaluate_daclip.py:45-50, 78-84): probs[B][K] =
 * softmax_k(100 * <degra_b / |degra_b|, text_k / |text_k|>), argmax[B] = first maximum.
 * degra [B, E], text_features [K, E] fp32 device; K <= 64. */
int dac_degradation_probs(dac_handle* h, const float* degra, const float* text_features, int B, int K,
                          int E, float* probs, int32_t* argmax, void* stream);

/* One ConditionalUNet forward: eps = model(xt, mu, t, text_ctx, image_ctx), all [B,3,H,W]
 * except contexts [B,context_dim]; text_ctx / image_ctx may be NULL. */
int dac_unet_forward(dac_handle* h, const float* xt, const float* mu, float t,
                     const float* text_ctx, const float* image_ctx, int B, int H, int W,
                     float* eps_out, void* stream);

/* IR-SDE schedule. If `tables` is non-NULL it holds 4*(T+1) host floats
 * [thetas | sigmas | thetas_cumsum | sigma_bars] computed by the caller (bit-identical to the
 * reference's torch ops) and `dt` is used as given; otherwise the tables are computed here
 * in fp32 following sde_utils.py:91-154. */
int dac_sde_schedule(dac_handle* h, float max_sigma, int T, int schedule, float eps,
                     const float* tables, float dt);

/* Full reverse loop t = T..1 in place on x_inout [B,3,H,W] with mu = LQ [B,3,H,W].
 * noise: NULL -> device Philox N(0,1) keyed by (seed, step, element); else [T,B,3,H,W]
 * fp32 device tensor, slice i consumed at step t = T - i (parity mode). Captured once per
 * (B,H,W,T,mode, which contexts / noise are given) as a hipGraph and replayed; injected
 * noise is copied into a handle-owned buffer first, so the caller may free or reuse it.
 * text_ctx NULL skips the prompt embedding (DenoisingUNet_arch.py:133-137); image_ctx NULL
 * makes every SpatialTransformer's attn2 a self-attention (attention.py:174), which, as in
 * the reference, requires context_dim == channels at those levels (DAC_E_ARG otherwise). */
int dac_sde_reverse(dac_handle* h, int mode, float* x_inout, const float* mu,
                    const float* text_ctx, const float* image_ctx, int B, int H, int W, int T,
                    const float* noise, uint64_t seed, void* stream);

/* Tiled reverse loop for images larger than the network's training size: one full-image state
 * x_inout [B,3,H,W]; at every step t = T..1 the tiles of x (th x tw windows at the product of
 * the host offset lists ys[ny] x xs[nx], tile k = (b*ny + iy)*nx + ix) go through the UNet
 * tiles_per_forward at a time (each with the context rows of its image; a tile whose side is
 * not a multiple of the padding unit is reflect-padded like a stand-alone image), the per-tile
 * eps are blended to a full-image eps and the sampler update of dac_sde_reverse acts on the full
 * image with the full-image noise (injected [T,B,3,H,W], or Philox keyed by the full-image
 * element under the dac_set_noise_offset rule), so a pixel's noise does not depend on the tiling.
 * Blend: a pixel inside exactly one tile takes that tile's value unchanged (a one-tile grid
 * reproduces dac_sde_reverse bit for bit); otherwise (sum_k w_k eps_k) / (sum_k w_k) over the
 * covering tiles in ascending k, w = wy * wx with the per-axis weight min(i + 1, l - i,
 * overlap + 1) at position i of a tile side l; fp32, multiply and add rounded separately, one
 * division, no atomics. The result does not depend on tiles_per_forward.
 * DAC_E_ARG before any device work: a null or empty offset list; th or tw < 2 or larger than
 * the image; overlap < 0 or >= min(th, tw); an offset out of bounds or not ascending; an axis
 * the tiles do not cover; tiles_per_forward < 1. DAC_E_STATE while profiling is enabled.
 * The loop is captured as one hipGraph per (shape, grid contents, tiles per forward, T, mode,
 * which contexts / noise are given); a loop of more than 65536 graph nodes is enqueued eagerly
 * on the handle's stream instead, with the same launches and so the same result. */
int dac_sde_reverse_tiled(dac_handle* h, int mode, float* x_inout, const float* mu,
                          const float* text_ctx, const float* image_ctx, int B, int H, int W,
                          int th, int tw, int overlap, const int32_t* ys, int ny,
                          const int32_t* xs, int nx, int tiles_per_forward, int T,
                          const float* noise, uint64_t seed, void* stream);

/* Op-level test hook: the blend of dac_sde_reverse_tiled on its own, handle-less (the caller
 * owns the memory; everything on the current device). eps_tiles [B*ny*nx,3,th,tw] ->
 * eps_full [B,3,H,W], fp32; ys / xs are host arrays. DAC_E_ARG for the grids
 * dac_sde_reverse_tiled refuses. Synchronises the stream before it returns. */
int dac_op_tile_blend(const float* eps_tiles, float* eps_full, int B, int H, int W, int th, int tw,
                      int overlap, const int32_t* ys, int ny, const int32_t* xs, int nx,
                      void* stream);

/* Device-noise keying for sharded runs: with noise == NULL, element e of image b draws
 * Philox(seed, step, (first_image + b) * 3*H*W + e), so a shard whose first global image is
 * `first_image` reproduces exactly the noise that image receives in an unsharded batch
 * (results are independent of the world size). Default 0. */
int dac_set_noise_offset(dac_handle* h, uint64_t first_image);

/* Time fed to the model at step t: t * scale, with scale = IRSDE.sample_scale = T / sample_T
 * (utils/sde_utils.py:86-88, 266, 302: noise_fn(x, t, self.sample_scale)). Default 1. The
 * product is formed in double and rounded once to float32, like the reference's python float
 * becoming torch.tensor([time]) (DenoisingUNet_arch.py:120-121). */
int dac_sde_set_time_scale(dac_handle* h, double scale);

/* One sampler update given the model output: x <- step(x, eps, t, z); x, eps, mu, z are
 * [B,3,H,W] fp32 and n = B*3*H*W elements (must be a multiple of 3). */
int dac_posterior_step(dac_handle* h, int mode, float* x_inout, const float* eps,
                       const float* mu, const float* z, int t, int n, void* stream);

/* Workload model: algorithmic FLOPs of one UNet forward at (B,H,W) and of one encode,
 * counted 2*MAC over conv/linear/bmm like torch.utils.flop_counter. */
double dac_unet_flops(dac_handle* h, int B, int H, int W);
double dac_encode_flops(dac_handle* h, int B);

/* Kernel timing over the next dac_sde_reverse call: HIP events around every launch of
 * the dominant conv class (`kernel_id` = 0), on the stream it runs on. Returns the
 * number of timed launches and their mean duration (ms) / flops per launch. */
int dac_profile_enable(dac_handle* h, int kernel_id);
int dac_profile_read(dac_handle* h, double* mean_ms, double* flops_per_launch,
                     double* bytes_per_launch);
/* graph_stamps = 1: the profiled dac_sde_reverse records its loop into a captured graph exactly
 * as the timed loop (side-stream branches included) with a wall-clock [begin, end] stamp pair
 * written by every launch of the class (kernel_id 999 = every conv launch), replays it once and
 * reads each launch's in-graph duration (HIP events cannot be timed inside graph replays);
 * 0 (default) = the eager replay with an event pair around each launch. */
int dac_profile_mode(dac_handle* h, int graph_stamps);
/* Launch i of the last profile (after dac_profile_read): duration (ms), algorithmic flops and
 * bytes, conv class (kh*100 + variant), (graph mode) start time in ms after the replay's first
 * profiled launch (-1 in eager mode), whether it ran in a concurrent branch of the UNet's split
 * section, its shape label and (graph mode) the kernel symbol. */
int dac_profile_launch(dac_handle* h, int i, double* ms, double* flops, double* bytes, int* kernel_class,
                       double* start_ms, int* in_branch, char* label, int label_len, char* symbol,
                       int symbol_len);
/* Graph mode: HIP-event time (ms) of the profiled graph replay on the loop's stream. */
int dac_profile_graph_ms(dac_handle* h, double* ms);

/* Op-level test hook: the SpatialTransformer self-attention core on its own (the kernel
 * dac_unet_forward runs for attention.py:170-193). qkv is [B*L, 3*H*32] (q | k | v, heads
 * of 32), out [B*L, H*32], both in `dtype` (DAC_F32 / DAC_BF16) on the current device;
 * scale = 32^-0.5. variant: 0 = the dispatcher's choice, 1 = the staged-tile kernel,
 * 2 = the K/V-ring kernel (16-bit dtypes, L % 64 == 0; DAC_E_ARG otherwise), 3 = the 16-wave
 * K/V-resident kernel (16-bit dtypes, L % 256 == 0, L <= 1024; DAC_E_ARG otherwise), 4 = the
 * same with its two query groups per wave walked jointly (prescaled q and L % 512 == 0; other
 * shapes run as 3; same constraints as 3).
 * variant | DAC_ATTN_Q_PRESCALED: q was multiplied by 32^-0.5 * log2(e) before rounding (as the
 * 16-bit handles' q|k|v weights are), so scores come out in log2 units.
 * dtype: DAC_F32, DAC_BF16 or DAC_F16. */
enum { DAC_ATTN_Q_PRESCALED = 8 };
int dac_op_attention(const void* qkv, void* out, int B, int L, int H, int dtype, int variant,
                     void* stream);

/* Op-level test hooks: the LinearAttention kernels on their own, handle-less (the caller owns
 * x / y / the weights; everything on the current device). Both allocate their scratch, run on
 * `stream`, synchronise it and free the scratch before they return.
 *
 * dac_op_linear_attention: the fused block Residual(PreNorm(LinearAttention)) exactly as the
 * engine launches it: y = x + LN(to_out(ctx^T softmax_d(q))) * gout. x, y: [B*HW, C] in `dtype`;
 * wqkv: to_qkv [384][C] in `dtype` (q | k | v rows, the PreNorm gain folded in); wout [C][128],
 * bout [C], gout [C]: fp32. qshift > 0: a bound on every |q|, used as the q-softmax shift (what
 * the engine derives from the weights when it is <= 40); 0: the per-pixel max.
 *
 * dac_op_linear_attention_weff: the unfused context chain on qkv [B*HW, 384] in `dtype`
 * (q | k | v): weff [B][C][128] in `dtype`, W_eff[b][c][h*32+d] = sum_e Wout[c][h*32+e]
 * ctx[b][h][d][e] / HW in the natural layout; hw_scale > 0 replaces the 1/HW (fp16 handles pass
 * S / HW, S the power of two >= HW).
 *
 * DAC_E_ARG, before any device work, for: a null pointer; B or HW < 1; C not in {64, 128, 256};
 * dtype not DAC_F32 / DAC_BF16 / DAC_F16; DAC_F32 with C = 256 (no fp32 kernel of that width);
 * a negative (or NaN) qshift / hw_scale. */
int dac_op_linear_attention(const void* x, const void* wqkv, const float* wout, const float* bout,
                            const float* gout, void* y, int B, int HW, int C, int dtype,
                            float qshift, void* stream);
int dac_op_linear_attention_weff(const void* qkv, const float* wout, void* weff, int B, int HW, int C,
                                 int dtype, float hw_scale, void* stream);

/* Op-level test hook: ONE conv / linear launch exactly as the dispatcher makes it (csrc/kernels.h
 * ConvArgs, csrc/conv_plan.h), handle-less: the caller owns every tensor, all on the current
 * device.   y[m, n] = epi(sum_k A[m, k] W[n, k]),  m = (b, oh, ow),  k = (kh, kw, ci)
 * with A the zero-padded (up = 1: 2x nearest-upsampled) NHWC input, channels [0, C1) from x1 (row
 * pitch ld1) and [C1, Cin) from x2 (ld2); epilogue +bias -> *(1 + scale) + shift -> act -> +res1 ->
 * +res2 -> +bbias. kh in {1, 3, 4, 7} fixes the window: 1x1 s1 p0, 3x3 s1 p1, 4x4 s2 p1, 7x7 s1 p3.
 * x1, x2, w, res1, res2, w_gs, y are in `dtype` (DAC_F32 / DAC_BF16 / DAC_F16); bias [Cout],
 * ss (scale [b*ss_ld + n], shift [b*ss_ld + Cout + n]), bbias [b*bb_ld + n] and b_gs are fp32.
 * w is [Cout][K] in the packed layout the kernels read (csrc/pack.h): K = kh*kw*Cin, the
 * 7x7 row-tap layout with kw padded to 8 (K = 7*8*Cin, twice that with cwrap = 1 for [hi rows |
 * lo rows]), or [hi Cin | lo Cin] per tap over an input read twice (x2 = x1, or cwrap = Cin / 2).
 * act: 0 none, 1 SiLU, 2 GELU, 3 GEGLU (w in the 16-row interleaved order, y has Cout / 2
 * columns; w_gs / b_gs: the same in the swapped-tile order, or null). ksplit > 1: split-K over
 * that many K ranges into an fp32 workspace the hook owns, then the reduce + epilogue pass.
 * conv3_force / conv2_force / conv2_force32: the selection knobs of csrc/conv_plan.h for this
 * call only (DAC_CONV_KEEP: leave the process's value); restored before the hook returns.
 * plan_out (DAC_CONV_PLAN_N ints, or null) receives the plan: kind (ConvKind), BM, BN, ST, epi,
 * fl, buffer_dma, label.
 * y == NULL: plan-only. plan_out is filled from the selection and nothing else happens: no HIP
 * call, so this mode works without a GPU (pointers are only tested for null / alignment).
 * Otherwise the hook owns the zero page and the split-K workspace, runs on `stream`,
 * synchronises it and frees its scratch on every path.
 * DAC_E_ARG, before any device work: a null descriptor, x1 or w; a dtype, kh, act or dimension
 * outside the above (B, Hs, Ws, Cin, Cout, K, ld*, ldy < 1 where used; Cin not a multiple of the
 * 16-byte vector; ksplit < 0); C1 < Cin without x2; res1 / res2 with a pitch below the output
 * width, ss / bbias with a negative one; or arguments for which the selection has no kernel
 * (kind 0). */
typedef struct dac_conv_desc {
  int dtype, kh;
  int B, Hs, Ws, up;
  int C1, Cin, ld1, ld2;
  int Cout, K, ldy;
  int act, cwrap, ksplit;
  int ss_ld, ldr1, ldr2, bb_ld;
  int conv3_force, conv2_force, conv2_force32;
} dac_conv_desc;
enum { DAC_CONV_KEEP = -1000, DAC_CONV_PLAN_N = 8 };
int dac_op_conv(const dac_conv_desc* d, const void* x1, const void* x2, const void* w, const float* bias,
                const float* ss, const void* res1, const void* res2, const float* bbias, const void* w_gs,
                const float* b_gs, void* y, int* plan_out, void* stream);

/* Op-level test hook: dac_op_conv with the two ConvArgs features only the stride-1 3x3 kernels
 * have. Everything dac_op_conv documents holds unchanged (operands, plan-only mode with
 * y == NULL, plan_out, the knob override and its restore, the hook-owned zero page and split-K
 * workspace, stream synchronisation, scratch freed on every path); e == NULL is dac_op_conv.
 *   Fused second output (the ResBlock's 1x1 res_conv, csrc/kernels.h ConvArgs::w2 / y2):
 *     y2[m, n] = sum_c x[m, c] w2[n, c] over the same (x1 | x2) input at the centre tap, no
 *     epilogue; w2 is [Cout][Cin] and y2 has row pitch e->ldy2, both in `dtype`. Served by conv3r
 *     (Cin 128) and the 16-bit C3I_RES v4 tiles, with the built-in selection (conv3_force < 0).
 *   e->uph in {0, 1, 2}: the row- (1) or row+column-phase (2) form of an up = 1 conv
 *     (ConvArgs::uph). w is then the DAC_PACK_UPH_ROW layout [Cout][4][3][Cin] (d->K = 12 Cin) or
 *     the DAC_PACK_UPH_COL layout [Cout][4][4][Cin] (d->K = 16 Cin) that dac_op_pack produces:
 *     output row 2i + a reads source rows i - 1 + a + s (s = 0, 1) with weight row set 2a + s;
 *     uph = 1 keeps the three column taps over the upsampled columns, uph = 2 folds them the same
 *     way (output column 2j + b reads source columns j - 1 + b + t with column set 2b + t).
 * In plan-only mode y2 is only tested for null, like every other pointer.
 * DAC_E_ARG, before any device work, for everything dac_op_conv refuses and: exactly one of w2 /
 * y2; w2 / y2 without e, or with e->ldy2 < Cout; uph outside {0, 1, 2}; uph without up = 1 (or kh
 * != 3); d->K not the uph layout's (12 Cin / 16 Cin; 9 Cin with uph = 0); uph together with
 * cwrap or ksplit; and any combination the selection answers with kind 0 (a fused output or a
 * phase form on a shape, dtype or forced configuration that has no such kernel). */
typedef struct dac_conv_ext {
  int uph;
  int ldy2;
} dac_conv_ext;
int dac_op_conv_ex(const dac_conv_desc* d, const dac_conv_ext* e, const void* x1, const void* x2, const void* w,
                   const float* bias, const float* ss, const void* res1, const void* res2, const float* bbias,
                   const void* w_gs, const float* b_gs, void* y, const void* w2, void* y2, int* plan_out,
                   void* stream);

/* Op-level test hook: the fused ResBlock kernel (csrc/rbfuse.hip, csrc/kernels.h RbArgs) as ONE
 * launch, handle-less: the caller owns every tensor, all on the current device.
 *   h = SiLU(conv3x3(x, w1) * (1 + scale) + shift),  y = SiLU(conv3x3(h, w2)) + res,
 *   res = x (Cin = 64) or x wr^T (Cin = 128); both convs zero-pad, h is zero outside the image.
 * x = (x1 | x2): channels [0, C1) from x1 (row pitch ld1), [C1, Cin) from x2 (ld2), NHWC rows of
 * B * H * W pixels; w1 [64][3][3][Cin], w2 [64][3][3][64], wr [64][Cin] (Cin = 128) or NULL
 * (Cin = 64); x, w and y (row pitch ldy, 64 channels) in `dtype` (DAC_BF16 / DAC_F16); ss fp32,
 * 16-byte aligned: scale [b * ss_ld + n], shift [b * ss_ld + 64 + n].
 * geom_out (2 ints, or null) receives the launch geometry: band height (output rows per block)
 * and strip width (output columns per block).
 * y == NULL: the served-query. Nothing touches the device (pointers are only tested for null /
 * alignment); returns 1 if rbfuse_ok takes these arguments (geom_out filled), 0 if not.
 * Otherwise runs on `stream`, synchronises it and returns DAC_OK.
 * DAC_E_ARG, before any device work: a null descriptor, x1, w1, w2 or ss; ss not 16-byte
 * aligned; a dtype other than the two 16-bit ones; B, H, W, C1, Cin < 1 (or above 2^24, or
 * B * H * W above 2^30); C1 < Cin without x2 or with ld2 < Cin - C1; ld1 below the channels read
 * from x1; ldy < 64; ss_ld < 0; and, with y != NULL, whatever rbfuse_ok refuses (Cin outside
 * {64, 128}; wr given with Cin = 64 or missing with Cin = 128; W below 256 or not a multiple of
 * the strip width, 128 columns at Cin 64 and 64 at Cin 128; two sources other than 64 | 64;
 * pitches that are not multiples of 8 elements; ss_ld not a multiple of 4; an image of 2^31 bytes
 * or more). */
typedef struct dac_rb_desc {
  int dtype;
  int B, H, W;
  int C1, Cin, ld1, ld2;
  int ss_ld, ldy;
} dac_rb_desc;
int dac_op_rbfuse(const dac_rb_desc* d, const void* x1, const void* x2, const void* w1, const void* w2,
                  const void* wr, const float* ss, void* y, int* geom_out, void* stream);

/* Host-only test hook: one weight-packing function of csrc/pack.h, the code dac_finalize_weights
 * packs with, on host arrays. No HIP call, so it works without a GPU. w (and gain / beta / bias
 * where the layout has them) are fp32 as a checkpoint stores them; `dtype` is the storage type
 * (DAC_BF16 / DAC_F16: uint16 bits; DAC_F32: the fp32 values before rounding; DAC_FP8 for the e4m3
 * layouts), `round` 0 = nearest even, 1 = the sum-keeping rounding over each (row, channel) group
 * of taps. need[3] always receives the outputs' byte sizes; out == NULL is the size query, else
 * out[i] / cap[i] are the buffers and their capacities for every need[i] > 0. Layouts (outputs):
 *   CODEC      w[O] -> bf16 / f16 / e4m3 element-wise; flag = 1: the codes decoded again (fp32)
 *   EMU_FP16   w[O] -> fp32 rounded to 11 significant bits (DAC_F32)
 *   CONV       w[O][C][kh][kw] -> [O][kh][kws][cin], cin = C up to 8 (16-bit) / 4, kws = max(kw, kwp)
 *   DUAL       ... -> split precision [O][kh][kw][hi cin | lo cin], kwp > kw: [O][hi rows | lo rows]
 *   UPH_ROW / UPH_COL   3x3 -> the row-phase [O][4][3][cin] / row+column-phase [O][4][4][cin] folds
 *   Q8C3       64x64x3x3 -> e4m3 [64][9][64], E8M0 [64][9][2]
 *   GEGLU / GEGLU_GS    w[2F][I], bias[2F] -> rows gathered (GS: F % 32 == 0, else F % 16 == 0);
 *              gathered bias (fp32); the source row of each packed row (int32)
 *   CONCAT     w[K][O][I] -> [K*O][I], the first block times `scale`
 *   TRANSPOSE  w[I][O] -> [O][I] (DAC_F32)
 *   FP8        w[O][K] -> e4m3 [O][Kp]; E8M0 [O][Kp/64]; Kp (int32), K up to a multiple of 128
 *   FOLD_LN    w[O][K], gain[K], beta[K] or NULL, bias[O] or NULL -> w' (16-bit); cs[O]; bias'[O]
 *   LA_FOLD    w[O][C] (first O/3 rows = q), gain[C] -> w diag(gain); qshift (fp32, 0 with flag = 0)
 * DAC_E_ARG before any buffer is touched: a null descriptor, need, w, required gain / bias, or
 * output; an unknown layout, dtype (or one the layout does not store) or round; a non-positive
 * dimension; a layout's precondition above; a capacity below the needed size. */
enum dac_pack_layout {
  DAC_PACK_CODEC = 0, DAC_PACK_EMU_FP16, DAC_PACK_CONV, DAC_PACK_DUAL, DAC_PACK_UPH_ROW, DAC_PACK_UPH_COL,
  DAC_PACK_Q8C3, DAC_PACK_GEGLU, DAC_PACK_GEGLU_GS, DAC_PACK_CONCAT, DAC_PACK_TRANSPOSE, DAC_PACK_FP8,
  DAC_PACK_FOLD_LN, DAC_PACK_LA_FOLD
};
typedef struct dac_pack_desc {
  int layout, dtype, round;
  int O, C, kh, kw, kwp;
  int F, I, K;
  int flag;
  float scale;
} dac_pack_desc;
int dac_op_pack(const dac_pack_desc* d, const float* w, const float* gain, const float* beta, const float* bias,
                void* const* out, const size_t* cap, size_t* need);

/* Evaluation metrics of config/daclip-sde/test.py:131-196 on the device, handle-less (the
 * caller owns all memory; everything on the current device). out / gt: fp32 [B,C,H,W] RGB,
 * C in {1, 3}. out_bytes / gt_bytes: uint8 [B,H,W,C], BGR for C = 3, what util.tensor2img
 * gives (clamp to [0,1], * 255 in fp32, round half to even); both are required, the metrics
 * read them. A non-finite input is stored as 0 and counted. results: double [B][8] =
 *   { sse, n, ssim, sse_y, n_y, ssim_y, nonfinite, reserved }
 * over the window cropped by crop_border on every side: sse = exact sum of squared byte
 * differences over all channels, n = its element count (PSNR = 20 log10(255 / sqrt(sse / n)),
 * infinite for sse == 0); ssim = mean of every channel's SSIM map (11x11 Gaussian window,
 * sigma 1.5, 'valid' region, C1 = (0.01*255)^2, C2 = (0.03*255)^2; utils/img_utils.py:192-234),
 * fp64; the _y entries are the same on Y = (24.966 B + 128.553 G + 65.481 R) / 255 + 16, kept
 * unrounded (data/util.py:189-210 on a float image), and 0 for C = 1; nonfinite = non-finite
 * values among the image's out and gt inputs. A record depends on neither B, the image's
 * place in the batch, nor the run (no atomics, fixed summation order).
 * workspace: dac_image_metrics_workspace(...) bytes of device scratch, 8-byte aligned.
 * DAC_E_ARG (before any device work): a null pointer, B < 1 (or > 16383), C not 1 or 3,
 * crop_border < 0, or a cropped height or width below 11; dac_image_metrics_workspace returns
 * 0 for the same shapes. The host metrics give NaN (with a numpy warning) for a window smaller
 * than the filter; this entry point refuses it instead. */
size_t dac_image_metrics_workspace(int B, int C, int H, int W, int crop_border);
int dac_image_metrics(const float* out, const float* gt, int B, int C, int H, int W, int crop_border,
                      unsigned char* out_bytes, unsigned char* gt_bytes, double* results,
                      void* workspace, void* stream);

const char* dac_last_error(dac_handle* h);

/* Build provenance baked in at compile time: "<sha256 of the library sources>[:16] git=<HEAD>"
 * (da-clip_amd/Makefile). The Python side recomputes the source hash from the tree, so a run
 * can prove which sources the loaded library was built from. */
const char* dac_build_id(void);

#ifdef __cplusplus
}
#endif
#endif /* DACLIP_HIP_H */
