/* pnpflow_hip.h -- C ABI of libpnpflow_hip.so, the MI355X (gfx950) engine behind the
 * PnP-Flow restoration hot path.
 *
 * The reference (annegnx/PnP-Flow) has no FFI layer: its hot path is Python calling
 * PyTorch ops.  This ABI is the boundary the build creates *below* the reference's
 * `pnpflow.methods` / `pnpflow.degradations` / `pnpflow.models.UNet` Python API; each
 * entry point cites the reference code it replaces (paths relative to the reference
 * repository root).  INTEGRATION.md shows the ctypes binding a maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success, a negative pf_status otherwise; no C++
 *     exception crosses the ABI; pf_last_error() gives the message of the last failure
 *     on that engine (or of pf_engine_create when called with NULL).
 *   - all tensor arguments are DEVICE pointers to contiguous fp32 NCHW buffers owned by
 *     the caller (what torch.Tensor.data_ptr() yields), unless named `host_*`.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); all work
 *     is enqueued on it, nothing synchronises the device except where stated.
 *   - one engine per device; an engine is not thread-safe.
 */
#ifndef PNPFLOW_HIP_H
#define PNPFLOW_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PF_ABI_VERSION 6

typedef enum pf_status {
    PF_OK = 0,
    PF_ERR_INVALID = -1,     /* bad argument / unsupported configuration */
    PF_ERR_HIP = -2,         /* a HIP runtime call failed */
    PF_ERR_WEIGHTS = -3,     /* unknown / missing / mis-shaped weight tensor */
    PF_ERR_STATE = -4,       /* call made in the wrong state (e.g. forward before finalize) */
    PF_ERR_NUMERIC = -5      /* a non-finite activation was detected inside the U-Net (see pf_engine_check_numerics) */
} pf_status;

typedef struct pf_engine pf_engine;

/* Hyper-parameters of pnpflow.models.UNet.__init__ (pnpflow/models.py:302-334);
 * define_model (pnpflow/utils.py:170-180) uses ch=32, ch_mult=(1,2,4,8),
 * num_res_blocks=6, attn_resolutions=(16,8). */
typedef struct pf_unet_cfg {
    int32_t input_channels;
    int32_t output_channels;
    int32_t input_height;      /* square images (the reference assumes it, utils.py:331) */
    int32_t ch;
    int32_t num_levels;
    int32_t ch_mult[8];
    int32_t num_res_blocks;
    int32_t num_attn_resolutions;
    int32_t attn_resolutions[8];
} pf_unet_cfg;


/* ---- NCSN++ ("rectified") velocity net ----------------------------------------------------
 * Hyper-parameters of pnpflow.image_generation.models.ncsnpp.NCSNpp.__init__ (ncsnpp.py:38-206) as the reference's two
 * rectified-flow configs set them (configs/rectified_flow/{celeba_hq,afhq_cat}_pytorch_rf_gaussian.py:46-64): BigGAN residual
 * blocks with FIR [1,3,3,1] resampling, input_skip / output_skip pyramids combined by `sum`, Gaussian Fourier time
 * conditioning, skip_rescale.  Only that block list is built (resblock_type 'biggan', progressive 'output_skip',
 * progressive_input 'input_skip', embedding 'fourier', conditional); nf must be a multiple of 32. */
typedef struct pf_ncsnpp_cfg {
    int32_t image_size;        /* config.data.image_size (256) */
    int32_t num_channels;      /* config.data.num_channels (3) */
    int32_t nf;                /* 128 */
    int32_t num_levels;        /* len(ch_mult) (7) */
    int32_t ch_mult[8];        /* (1,1,2,2,2,2,2) */
    int32_t num_res_blocks;    /* 2 */
    int32_t num_attn_resolutions;
    int32_t attn_resolutions[8];   /* (16,) */
    int32_t fir_taps;          /* len(fir_kernel) (4) */
    float fir_kernel[8];       /* [1,3,3,1] */
    int32_t skip_rescale;      /* 1 */
    int32_t scale_by_sigma;    /* 1: the output is divided by the time label (ncsnpp.py:378-381) */
    int32_t centered;          /* config.data.centered; 0: x -> 2x - 1 first (ncsnpp.py:248-250; not built: must be 1) */
} pf_ncsnpp_cfg;

/* replaces mutils.create_model(config) (models/utils.py:91-103).  The handle is a pf_engine: weights are loaded with
 * pf_engine_load_weight under NCSNpp's own state_dict keys ("all_modules.<i>.<...>", without DataParallel's "module."),
 * pf_unet_forward(e, x, labels, out, B, stream) is model(x, labels) with labels = the reference's time_cond (t * 999,
 * methods/pnp_flow.py:23-27); pf_unet_forward_retain / pf_unet_backward give its input-gradient VJP (ot_ode.py:137-138). */
int pf_ncsnpp_create(int device_id, const pf_ncsnpp_cfg* cfg, pf_engine** out);
/* label = t * scale inside pf_pnp_flow_restore / pf_ot_ode_restore (PNP_FLOW.model_forward: `t * 999`); 1 for the OT net */
int pf_engine_set_solver_time_scale(pf_engine* e, float scale);

int pf_abi_version(void);

/* ---- engine life cycle ------------------------------------------------------------ */
/* replaces UNet.__init__ + .to(device)  (pnpflow/models.py:302-436, methods/pnp_flow.py:15) */
int pf_engine_create(int device_id, const pf_unet_cfg* cfg, pf_engine** out);
void pf_engine_destroy(pf_engine* e);
const char* pf_last_error(const pf_engine* e);

/* replaces model.load_state_dict (pnpflow/utils.py:225): one call per state_dict entry,
 * `name` = the reference's key (e.g. "down_modules.3.3a_0b_attn.attn_q.weight"),
 * `host_data` = fp32 values in the reference's layout (OIHW / (out,in) / (C,)).
 * The engine repacks into its own device layout and owns the copy. */
int pf_engine_load_weight(pf_engine* e, const char* name, const float* host_data,
                          const int64_t* shape, int ndim);
/* checks that every tensor of the architecture was supplied; uploads. */
int pf_engine_finalize_weights(pf_engine* e);
/* number of state_dict entries the architecture expects, and the i-th name. */
int pf_engine_num_weights(const pf_engine* e);
const char* pf_engine_weight_name(const pf_engine* e, int i);
/* shape of the i-th entry (reference layout); returns the rank (<= 4) or a negative status. */
int pf_engine_weight_shape(const pf_engine* e, int i, int64_t shape[4]);

/* 1 (default) = split-fp16: every operand carried as an fp16 pair hi+lo, 3 x v_mfma_f32_32x32x16_f16 per product,
 *     fp32 accumulate - fp32-equivalent results (the parity tests hold both modes to the same tolerance) at 3/16 of
 *     the matrix-pipe time.  Applies to the packed-weight convs of the forward and of the backward (the VJP input is
 *     normalised by a power of two first) and selects the fused attention core (q k^T, softmax, P v in one launch)
 *     where its shapes apply; the unfused attention matmuls and their adjoints run on the fp32 MFMA.
 * 0 = exact fp32 MFMA (v_mfma_f32_32x32x2_f32) everywhere.
 * 2 = single fp16 MFMA per product: the packed-weight convs round both operands to fp16 (11-bit significands; the per-image
 *     power-of-two operand scales keep them in range) and accumulate in fp32 - the precision class of the TF32 convolutions the
 *     reference's CUDA runs use by PyTorch default (torch.backends.cudnn.allow_tf32), NOT fp32-equivalent: U-Net outputs
 *     agree with the fp32 reference to ~1e-3 relative, restored images to the +-0.05 dB PSNR the BASELINE tolerance asks. */
int pf_engine_set_precision(pf_engine* e, int mode);

/* ---- velocity field ---------------------------------------------------------------- */
/* replaces UNet.forward (pnpflow/models.py:442-495) as called by PNP_FLOW.model_forward
 * (pnpflow/methods/pnp_flow.py:19-21):  v[B,Cout,H,W] = v_theta(x[B,Cin,H,W], t[B]). */
int pf_unet_forward(pf_engine* e, const float* x, const float* t, float* v, int B, void* stream);

/* debugging / parity localisation: copy an internal NHWC activation (by plan tensor
 * index) of the last forward to a HOST fp32 buffer in NCHW order; returns C*H*W via
 * dims[3] = {C,H,W}.  Synchronises the stream. */
int pf_engine_num_taps(const pf_engine* e);
const char* pf_engine_tap_name(const pf_engine* e, int i);
int pf_engine_read_tap(pf_engine* e, int i, float* host_out, int64_t capacity, int32_t dims[3], void* stream);

/* ---- degradation operators (pnpflow/degradations.py) -------------------------------- */
typedef enum pf_degradation_kind {
    PF_DEG_DENOISING = 0,       /* Denoising           degradations.py:15-20  */
    PF_DEG_BOX_INPAINTING = 1,  /* BoxInpainting       degradations.py:23-32, utils.py:327-336 */
    PF_DEG_MASK_INPAINTING = 2, /* RandomInpainting    degradations.py:35-44 (mask supplied: utils.py:353-361) */
    PF_DEG_SUPERRESOLUTION = 3, /* Superresolution     degradations.py:92-127, mode=None, utils.py:283-310 */
    PF_DEG_GAUSSIAN_BLUR = 4,   /* GaussianDeblurring  degradations.py:55-89 (circular, separable) */
    PF_DEG_SR_FILTERED = 5,     /* Superresolution mode="bicubic": circular separable filter (utils.py:365-396), then decimation
                                   degradations.py:97-127; uses sf, ntaps (4*sf, even), taps */
    PF_DEG_GAUSSIAN_BLUR_ZERO = 6,/* GaussianDeblurring, any mode but "fft" (degradations.py:72-76, 82-86): F.conv2d(padding='same'), i.e. the
                                   correlation with outer(taps, taps) where samples outside the image are 0; H_adj is the matching convolution
                                   (= H for the symmetric Gaussian).  Same fields as GAUSSIAN_BLUR (ntaps, taps) */
    PF_DEG_PSF_BLUR = 7,        /* circular blur with any square 2-D point-spread function (what the reference computes when GaussianDeblurring's
                                   `.filter` holds the PSF, degradations.py:62-89): H is the circular convolution y[i] = sum_j k[j] x[i - (j - r)],
                                   r = K/2 on both axes, H_adj the circular correlation.  ntaps = K, the side of the K x K PSF; taps: device [K][K] row-major */
    PF_DEG_PSF_BLUR_ZERO = 8,   /* the same PSF where samples outside the image are 0: H is the correlation (F.conv2d(padding='same')), H_adj the
                                   convolution - the true adjoint, which the reference's own spatial H_adj is not for an asymmetric kernel.
                                   Same fields as PSF_BLUR */
    PF_DEG_PSF_SR = 9           /* superresolution through a blur kernel, y = (k (*) x) decimated by sf: H is the circular convolution of PSF_BLUR sampled at
                                   (i sf, j sf), H_adj the zero-fill followed by the circular correlation - what the reference's Superresolution(mode="bicubic")
                                   computes when its `.filter` holds the PSF (degradations.py:113-127).  Fields: sf, ntaps = K, taps: device [K][K]; x == y is refused.
                                   H H^T is circulant on the low-resolution grid (pf_sr_aliased_spectrum), which gives OT-ODE and the hqs prox one Fourier solve */
} pf_degradation_kind;

/* When a descriptor may be applied to [B,C,H,W] images.  Every entry point that takes a pf_degradation checks these rules on the host and returns
 * PF_ERR_INVALID before anything is launched (the solvers: with a pf_last_error text under their prefix, before anything is allocated):
 *
 *   any kind                                    0 <= kind <= 9
 *   MASK_INPAINTING                             mask != NULL
 *   SUPERRESOLUTION, SR_FILTERED, PSF_SR        sf >= 1, H % sf == 0, W % sf == 0
 *   GAUSSIAN_BLUR, SR_FILTERED,                 taps != NULL, 1 <= ntaps <= 127; no rule between ntaps and the image side
 *     GAUSSIAN_BLUR_ZERO
 *   PSF_BLUR, PSF_BLUR_ZERO, PSF_SR             taps != NULL, K = ntaps odd, 1 <= K <= 63; PSF_BLUR and PSF_SR: K <= min(H, W) (the circular filter
 *                                               must hold the kernel); PSF_SR: sf <= 8
 *
 * The Fourier solves (pf_ot_ode_vec and pf_ot_ode_restore with GAUSSIAN_BLUR, PSF_BLUR, SR_FILTERED or PSF_SR; pf_sr_aliased_spectrum, pf_sr_prox) also need
 * H, W <= 2048 and, for the separable filters, ntaps <= min(H, W).  What a single solver asks beyond this is written at its entry point. */

typedef struct pf_degradation {
    int32_t kind;
    int32_t half_size_mask;     /* BOX */
    int32_t sf;                 /* SUPERRESOLUTION, SR_FILTERED, PSF_SR */
    int32_t ntaps;              /* GAUSSIAN_BLUR / GAUSSIAN_BLUR_ZERO / SR_FILTERED: <= 127; tap ntaps/2 sits at offset 0 (the reference's roll by -(K-1)//2).
                                   PSF_BLUR / PSF_BLUR_ZERO / PSF_SR: the side K of the square PSF; tap (K/2, K/2) sits at offset (0, 0) */
    const uint8_t* mask;        /* MASK: device [B][H][W] bytes, 1 = keep */
    const float* taps;          /* GAUSSIAN_BLUR / GAUSSIAN_BLUR_ZERO / SR_FILTERED: device [ntaps] separable 1-D taps;
                                   PSF_BLUR / PSF_BLUR_ZERO / PSF_SR: device [ntaps][ntaps] row-major 2-D taps */
} pf_degradation;

/* y = H(x)      x:[B,C,H,W] -> y:[B,C,Hy,Wy]  (Hy = H/sf for SR, else H) */
int pf_degradation_H(const pf_degradation* d, const float* x, float* y, int B, int C, int H, int W,
                     float* scratch, void* stream);
/* x = H_adj(y) */
int pf_degradation_H_adj(const pf_degradation* d, const float* y, float* x, int B, int C, int H, int W,
                         float* scratch, void* stream);

/* ---- PnP-Flow iteration pieces (pnpflow/methods/pnp_flow.py) ------------------------- */
/* z = x - coef[b] * H_adj(H(x) - y),  coef[b] = lr_t[b] / sigma^2
 * replaces grad_datafit + the update at pnp_flow.py:39-41, 109-112 (gaussian noise).
 * scratch: >= 2*B*C*H*W floats for GAUSSIAN_BLUR, GAUSSIAN_BLUR_ZERO and SR_FILTERED (pf_degradation_H/H_adj: B*C*H*W resp. 2*B*C*H*W); >= B*C*H*W floats
 * for PSF_BLUR and PSF_BLUR_ZERO (the residual between the two applications; their pf_degradation_H/H_adj need none and refuse x == y); >= B*C*H*W / sf^2
 * floats for PSF_SR (the low-resolution residual; H / H_adj need none); may be NULL otherwise. */
int pf_grad_step(const pf_degradation* d, const float* x, const float* y, const float* coef, float* z,
                 int B, int C, int H, int W, float* scratch, void* stream);
/* Laplace noise model (pnp_flow.py:42-43): z = x - coef[b] * H_adj(2*heaviside(H(x) - y, 0) - 1), coef[b] = lr_t[b]/sigma */
int pf_grad_step_laplace(const pf_degradation* d, const float* x, const float* y, const float* coef, float* z,
                         int B, int C, int H, int W, float* scratch, void* stream);
/* z_tilde = t[b]*z + (1-t[b])*eps    (interpolation_step, pnp_flow.py:47-48)
 * eps = `noise` if non-NULL, else Philox4x32-10/Box-Muller (seed, stream_id). */
int pf_interpolate(const float* z, const float* t, const float* noise, uint64_t seed, uint64_t stream_id,
                   float* z_tilde, int B, int n_per_image, void* stream);
/* acc (=|+=) z_tilde + (1-t[b])*v ; final: acc = (acc + ...)*inv_count  (denoiser + average,
 * pnp_flow.py:50-52, 114-121).  mode: bit0 = first sample (overwrite), bit1 = last (scale). */
int pf_denoise_accumulate(float* acc, const float* z_tilde, const float* v, const float* t, int mode,
                          float num_samples, int B, int n_per_image, void* stream);
/* fills out[n] with engine normals (the same generator pf_interpolate uses). */
int pf_fill_normal(float* out, int64_t n, uint64_t seed, uint64_t stream_id, void* stream);
/* the same, starting at normal number `elem_offset` of the stream: out[i] = normal number elem_offset + i.  A shard of a
 * multi-GPU run that owns images [lo, hi) of the global batch draws elem_offset = lo*C*H*W, i.e. exactly the numbers a
 * single-device run at the global batch size draws for those images (replaces the one torch.randn_like(x) over the whole
 * batch of interpolation_step, pnpflow/methods/pnp_flow.py:47-48, when the batch is split over GPUs). */
int pf_fill_normal_at(float* out, int64_t n, uint64_t seed, uint64_t stream_id, uint64_t elem_offset, void* stream);
/* fills out[n] with +-1.0f (Rademacher) from the same Philox4x32-10 words: out[i] = element e = elem_offset + i of the stream, which is
 * word e % 4 of counter (e/4 lo, e/4 hi, stream_id lo, stream_id hi) under key (seed lo, seed hi); +1 when the word's top bit is set, else -1.
 * Replaces torch.randint_like(data, low=0, high=2).float() * 2 - 1 (pnpflow/utils.py:251, image_generation/likelihood.py:168). */
int pf_fill_rademacher(float* out, int64_t n, uint64_t seed, uint64_t stream_id, uint64_t elem_offset, void* stream);

/* per-image PSNR of postprocess(rec) vs postprocess(clean), data_range 1
 * (pnpflow/utils.py:560-577, 594-611) -> out[B] (device). */
int pf_psnr(const float* rec, const float* clean, float* out, int B, int n_per_image, void* stream);

/* per-image SSIM of postprocess(rec) vs postprocess(clean): ignite.metrics.SSIM(data_range=1.0) as the reference calls it
 * (pnpflow/utils.py:780-802) - 11x11 Gaussian window sigma 1.5, k1 0.01, k2 0.03, reflect padding, mean over (C,H,W) in
 * fp64 -> out[B] (device, double).  H, W > 5.  PARITY UNPINNED: ignite is absent from the build container. */
int pf_ssim(const float* rec, const float* clean, double* out, int B, int C, int H, int W, void* stream);

/* ---- LPIPS (AlexNet, v0.1), SURVEY 8f N2 ------------------------------------------------------------------------------------
 * What the reference logs next to PSNR / SSIM (pnpflow/utils.py:677-724): lpips.LPIPS(net='alex')(img0, img1, normalize=True).
 * The network (torchvision AlexNet features + lpips' five 1x1 "lin" heads) is restated in csrc/lpips.hip; weights are loaded under
 * the published names "features.{0,3,6,8,10}.{weight,bias}" (torchvision.models.alexnet) and "lin{0..4}" (the [1][C][1][1] conv of
 * lpips' NetLinLayer, as [C]).  PARITY UNPINNED: neither package nor their weight files are in the build image. */
typedef struct pf_lpips pf_lpips;
int pf_lpips_create(int device_id, pf_lpips** out);
void pf_lpips_destroy(pf_lpips* l);
const char* pf_lpips_last_error(const pf_lpips* l);
int pf_lpips_load_weight(pf_lpips* l, const char* name, const float* host_data, const int64_t* shape, int ndim);
/* img0, img1: [B][3][H][W] fp32 on the device; out[B] (device) <- LPIPS distance per image pair.  normalize != 0 applies the
 * package's 2x - 1 first (the reference passes normalize=True on images that already are in [-1, 1]: utils.py:703-708). */
int pf_lpips_forward(pf_lpips* l, const float* img0, const float* img1, float* out, int B, int H, int W, int normalize, void* stream);

/* ---- FID Inception features (additive: PF_ABI_VERSION unchanged) ----------------------------------------------------------------
 * The feature network of the reference's FID (pnpflow/models.py:498-820: InceptionV3 on pytorch-fid's fid_inception_v3, eval mode),
 * restated in csrc/inception.hip from the layer table of csrc/inception_plan.h.  PARITY UNPINNED for the network: torchvision and the
 * published weight file are not in the build image.  The statistics and the Frechet distance on top live in pnpflow_amd/fid_score.py. */
typedef struct pf_inception pf_inception;
int pf_inception_create(int device_id, pf_inception** out);
void pf_inception_destroy(pf_inception* h);
const char* pf_inception_last_error(const pf_inception* h);
/* The layer table (host only, no device needed): layer `index` of pf_inception_num_layers, its name and
 * dims[7] = (Cin, Cout, KH, KW, stride, pad_h, pad_w). */
int pf_inception_num_layers(void);
int pf_inception_layer(int index, char* name, int name_cap, int32_t* dims);
/* The published state_dict names (models.py:694-695 loads them): "<layer>.conv.weight" [Cout][Cin][KH][KW] and
 * "<layer>.bn.{weight,bias,running_mean,running_var}" [Cout], <layer> e.g. "Conv2d_1a_3x3" or "Mixed_6c.branch7x7dbl_3".  The conv
 * weights are repacked and the BatchNorm (eps 1e-3) is folded into a scale and a shift here, once.  Unknown name / wrong shape:
 * PF_ERR_WEIGHTS. */
int pf_inception_load_weight(pf_inception* h, const char* name, const float* host_data, const int64_t* shape, int ndim);
/* InceptionV3.forward (models.py:617-651) followed by the spatial average of fid_score.py:60-65: img [B][3][H][W] fp32 on the device,
 * values in (0, 1) when normalize_input; out [B][dims] on the device, dims = 64 / 192 / 768 / 2048 for output_block 0..3.
 * resize_input: bilinear to 299 x 299 (align_corners=False).  Without it a side below 75 is refused with PF_ERR_INVALID and a message
 * (nothing is launched); a missing weight is PF_ERR_STATE.  Activation buffers are planned per (B, H, W) and regrown when a call needs
 * more.  Asynchronous on `stream`. */
int pf_inception_forward(pf_inception* h, const float* img, float* out, int B, int H, int W, int resize_input, int normalize_input, int output_block,
                         void* stream);
/* HIP-event time of every launch of the following forwards (they then synchronise `stream`); read back launch `index` of the last one
 * (PF_ERR_INVALID past the end): its layer name (or "front", "maxpool", "avgpool", "global_average"), milliseconds and
 * floating-point operations (2 M K Cout of a conv, 0 otherwise). */
int pf_inception_profile(pf_inception* h, int enable);
int pf_inception_profile_read(pf_inception* h, int index, char* name, int name_cap, float* ms, double* flops);
/* One launch of the network's conv kernel, for tests (one BasicConv2d of models.py:498-820 with the BatchNorm already folded):
 * in NHWC [B][Hi][Wi][Cin] (device), host_weight [Cout][Cin][KH][KW] (HOST; packed and uploaded here), scale / shift [Cout] (device),
 * out NHWC [B][Ho][Wo][out_cs] (device): channels [out_off, out_off + Cout) <- relu(conv * scale + shift), the others untouched.
 * tile: 0 128x128, 1 128x64, 2 64x128, 3 64x64 (pixels x channels per workgroup), negative: the planner's choice.  Cout % 4 == 0.
 * Synchronises `stream`. */
int pf_inception_conv(const float* in, const float* host_weight, const float* scale, const float* shift, float* out, int B, int Hi, int Wi, int Cin, int Cout,
                      int KH, int KW, int stride, int pad_h, int pad_w, int out_off, int out_cs, int tile, void* stream);
/* The network's 3 x 3 pools on channel slices of NHWC tensors (device), for tests.  kind 1: max, stride 2, no pad; 2: average, stride 1,
 * pad 1, count_include_pad=False (models.py:715-718); 3: max, stride 1, pad 1 (models.py:812-816). */
int pf_inception_pool(const float* in, float* out, int B, int C, int Hi, int Wi, int kind, int in_off, int in_cs, int out_off, int out_cs, void* stream);
/* The front end (models.py:634-641), for tests: img NCHW [B][3][H][W] -> out NHWC [B][299 | H][299 | W][3]. */
int pf_inception_front(const float* img, float* out, int B, int H, int W, int resize_input, int normalize_input, void* stream);

/* ---- the reference's native ops (NCSN++ "rectified" velocity net) ------------------------------------------- */
/* upfirdn2d (pnpflow/image_generation/op/upfirdn2d_kernel.cu:49-369; definition: op/upfirdn2d.py:142-187): per plane of
 * in[planes][in_h][in_w]: zero-insert upsample by (up_x, up_y), pad (negative = crop) by (pad_x0, pad_x1, pad_y0, pad_y1), true 2-D
 * convolution with kernel[kh][kw] (device), decimate by (down_x, down_y) -> out[planes][out_h][out_w],
 * out_h = (in_h*up_y + pad_y0 + pad_y1 - kh) / down_y + 1 (same for w). */
int pf_upfirdn2d(const float* in, const float* kernel, float* out, int planes, int in_h, int in_w, int kh, int kw, int up_x, int up_y,
                 int down_x, int down_y, int pad_x0, int pad_x1, int pad_y0, int pad_y1, void* stream);
/* fused_bias_act (op/fused_bias_act_kernel.cu:19-99): out[i] = act(x[i] + bias[(i / step_b) % size_b]) * scale;
 * act 1 = linear, 3 = leaky ReLU(alpha); grad 0 = value, 1 = first derivative (sign taken from ref[i], the saved output),
 * 2 = zero; bias / ref may be NULL. */
int pf_fused_bias_act(const float* x, const float* bias, const float* ref, float* out, int64_t n, int step_b, int size_b, int act, int grad,
                      float alpha, float scale, void* stream);

/* ---- attention core -------------------------------------------------------------------- */
/* out[B,T,C] = softmax(q k^T * C^-1/2, dim=-1) v for q|k|v stacked as qkv[B,T,3C] (fp32, token-major): the bmm /
 * softmax / bmm of SelfAttention.forward (pnpflow/models.py:152-158) in one launch, split-f16 MFMA (fp32-equivalent).
 * Shapes: T in {128, 256, 512, 768, ... 4096}, C in {128, 256}; anything else returns PF_ERR_INVALID (the engine then
 * uses three launches). */
int pf_attention_core(const float* qkv, float* out, int B, int T, int C, void* stream);
/* The same core with every option of the engine's launch (additive: PF_ABI_VERSION unchanged):
 *   kv_packed != 0   the k and v thirds of qkv hold, per element, the 32-bit word hi | lo << 16 of two fp16 values,
 *                    hi = RNE16(x), lo = RNE16(x - hi), in place of the fp32 value (q stays fp32);
 *   residual[B,T,C]  the folded output projection: out = (P v + bias[c]) + residual (bias[C] may be NULL = 0);
 *   stats_part       fp32 scratch [B][T/32][C][2] and stats double [B][C][2]: per image and channel the (sum, sum of
 *                    squares) of out over the tokens, 32-token tiles in fp32, tiles added in order in fp64 (deterministic).
 * Operand contract: finite results need |q|, |k|, |v| <= 65504; the error is 2e-5 max|P v| + 2^-24 absolute.
 * PF_ERR_INVALID with nothing launched for: the shapes pf_attention_core refuses, NULL qkv / out, B <= 0, bias or
 * stats_part without residual, one of stats_part / stats without the other, out == residual. */
int pf_attention_core_ex(const float* qkv, float* out, int B, int T, int C, const float* bias, const float* residual, float* stats_part, double* stats,
                         int kv_packed, void* stream);

/* ---- vector-Jacobian product (OT-ODE) ------------------------------------------------ */
/* replaces torch.autograd.functional.vjp(lambda z: model(z, t), x, vec) at
 * pnpflow/methods/ot_ode.py:137-138.  pf_unet_forward_retain = a forward that keeps every
 * activation; pf_unet_backward = J^T vec at the last retained forward (input gradient only);
 * pf_unet_vjp = both (v: the forward output, g: J^T vec). */
int pf_unet_forward_retain(pf_engine* e, const float* x, const float* t, float* v, int B, void* stream);
int pf_unet_backward(pf_engine* e, const float* vec, float* g, int B, void* stream);
int pf_unet_vjp(pf_engine* e, const float* x, const float* t, const float* vec, float* v, float* g, int B, void* stream);

/* OT-ODE linear solve + adjoint (pnpflow/methods/ot_ode.py:72-130) and Euler update (:141-147).
 *   vec = H_adj( (rt2[b] H H^T + sigma2)^-1 (y - H(x + one_minus_t[b]*vt)) )
 *   x  += delta * (vt + coef[b] * (vec + one_minus_t[b]*g)),  coef = ((1-t)/t)*gamma
 * Closed form per pixel where H H^T is diagonal (denoising, masks, decimation: ot_ode.py:81-106); for
 * GAUSSIAN_BLUR the Fourier-domain solve of ot_ode.py:108-117 with a hand-written 2-D FFT, which needs
 * scratch >= 4*B*C*H*W + H + W floats (H, W <= 2048); PSF_BLUR takes the same solve with the 2-D table of pf_psf_power_spectrum and needs
 * scratch >= 4*B*C*H*W + H*W floats; scratch may be NULL for the other operators.  GAUSSIAN_BLUR_ZERO and PSF_BLUR_ZERO have no closed form
 * (pf_krylov_solve) and return PF_ERR_INVALID.
 * SR_FILTERED and PSF_SR (blur, then decimate): H H^T is circulant on the low-resolution grid, so the solve is the same three FFT launches on
 * [H/sf][W/sf] with the aliased spectrum of pf_sr_aliased_spectrum:  vec = H_adj( ifft2_l( fft2_l(y - H(x1)) / (rt2 lam + sigma2) ) ).
 * scratch >= pf_sr_solve_scratch_floats(B, C, H, W, sf) floats (4-byte alignment is enough: the complex plane is placed at an 8-byte boundary inside); H, W <= 2048. */
int pf_ot_ode_vec(const pf_degradation* d, const float* x, const float* vt, const float* y, const float* one_minus_t,
                  const float* rt2, float sigma2, float* vec, int B, int C, int H, int W, float* scratch, void* stream);
int pf_ot_ode_update(float* x, const float* vt, const float* vec, const float* g, const float* one_minus_t,
                     const float* coef, float delta, int B, int n_per_image, void* stream);
/* pw2[H][W] (device floats) <- |fft2(filter)|^2 of a PF_DEG_PSF_BLUR operator, the filter being the PSF zero-padded to H x W and rolled so that
 * tap (K/2, K/2) sits at (0, 0) - the reference's `.filter` (degradations.py:62-68) - by a two-stage fp64 DFT of the K x K taps (along x, then
 * along y).  What the Fourier solves divide by (ot_ode.py:108-118, pnp_gs.py:35-44); the engine's loops compute it once per call.  H, W <= 2048. */
int pf_psf_power_spectrum(const pf_degradation* d, int H, int W, float* pw2, void* stream);
/* lam[H/sf][W/sf] (device floats) <- the eigenvalues of the circulant H H^T of a PF_DEG_PSF_SR or PF_DEG_SR_FILTERED operator,
 *   lam[u][v] = 1/sf^2 sum_{a, b < sf} |fft2(filter)|^2 [u + a H/sf][v + b W/sf],
 * folded in fp64 from the 2-D table of pf_psf_power_spectrum (PSF_SR) or from the two separable factors (SR_FILTERED).
 * tmp: device scratch of H*W floats (PSF_SR) or 2 (H + W) + 2 floats (SR_FILTERED: the folded factors are kept in fp64).  H, W <= 2048. */
int pf_sr_aliased_spectrum(const pf_degradation* d, int H, int W, float* lam, float* tmp, void* stream);
int64_t pf_sr_solve_scratch_floats(int B, int C, int H, int W, int sf);
/* The exact proximal map of alpha/2 |H x - y|^2 for PSF_SR / SR_FILTERED by the Woodbury identity on the low-resolution grid:
 *   out = in - alpha H_adj( ifft2_l( fft2_l(H in) / (alpha lam + 1) ) ),   in = z + alpha H_adj(y)  gives  out = prox(z).
 * alpha_dev: device double; lam: pf_sr_aliased_spectrum; scratch >= pf_sr_solve_scratch_floats floats; in != out.  Two calls return the same bits. */
int pf_sr_prox(const pf_degradation* d, const float* in, const double* alpha_dev, const float* lam, float* out, int B, int C, int H, int W, float* scratch,
               void* stream);

/* Batched GMRES on the device (the reference's utils.GMRES, pnpflow/utils.py:972-1109, as ot_ode.py:119-128 calls it), all images at once:
 *   (rt2[b] H H^T + sigma2 I) sol[b] = rhs[b]
 * from a zero initial guess, at most max_iter (<= 256) Krylov vectors, no restart; image b stops when |beta_{j+1}| < tol |rhs_b| or < atol;
 * |rhs_b| < 1e-8 returns rhs_b itself (utils.py:995-996).  Orthogonalisation: classical Gram-Schmidt with one re-orthogonalisation pass (two
 * multi-dot + update launch pairs per iteration); Hessenberg column, Givens rotations, beta and the per-image done flag stay on the device,
 * the host only polls the flags every 8 iterations to leave early (never under stream capture: max_iter masked iterations then).  Reductions
 * have a fixed order: two runs agree bit for bit.  Every kind whose measurement has the image's shape; the superresolution kinds return
 * PF_ERR_INVALID.  rt2_dev: device [B]; rhs, sol: device [B,C,H,W] (distinct); workspace: device, 16-byte aligned, workspace_floats >=
 * pf_krylov_workspace_floats(...) = (max_iter + 3) B C H W floats (basis + two operator temporaries) + the small per-image state;
 * iters_out_dev: device int32 [B] or NULL <- Krylov vectors in image b's solution (0 for the |rhs_b| < 1e-8 return). */
int64_t pf_krylov_workspace_floats(int B, int C, int H, int W, int max_iter);
int pf_krylov_solve(const pf_degradation* d, const float* rt2_dev, float sigma2, const float* rhs, float* sol, int B, int C, int H, int W,
                    int max_iter, float tol, float atol, float* workspace, int64_t workspace_floats, int32_t* iters_out_dev, void* stream);

/* Whole OT-ODE loop of one batch on the device (pnpflow/methods/ot_ode.py:63-147): iterations first..steps-1 of
 *   v_t = v_theta(x, t);  vec = H_adj((r_t^2 H H^T + sigma^2)^-1 (y - H(x + (1-t) v_t)));  g = J^T vec;
 *   x += delta * (v_t + coef * (vec + (1-t) g))
 * with the per-iteration scalars (host tables, fp32 values computed with the reference's own expressions - including its
 * `delta * iteration**2` quirk for superresolution, ot_ode.py:96) read on the device through an iteration counter, the buffers
 * pre-allocated, and one hipGraph per Euler step (retained forward -> solve -> hand-written backward -> update) captured once
 * and replayed.  GAUSSIAN_BLUR_ZERO has no closed form: its step is the reference's generic branch (ot_ode.py:119-128) - retained forward,
 * d = y - H(x + (1-t) v_t), pf_krylov_solve (max_iter 100, tol = atol = 1e-6; PSF_BLUR_ZERO takes the same path, PSF_BLUR the Fourier solve), vec = H_adj(sol), backward, update - as two captured halves with
 * the Krylov loop enqueued between them; pf_ot_ode_krylov_iterations reports how many Krylov iterations the last call enqueued.
 * x_inout: the initialisation t0*H_adj(y) + (1-t0)*noise on entry (ot_ode.py:27-28, 50-52), the result on exit. */
typedef struct pf_ot_ode_params {
    int32_t steps;                  /* steps_ode */
    int32_t first;                  /* int(steps_ode * start_time) */
    const float* host_t;            /* host [steps] */
    const float* host_one_minus_t;  /* host [steps] */
    const float* host_rt2;          /* host [steps] */
    const float* host_coef;         /* host [steps]: ((1-t)/t) * gamma_t */
    float sigma2;                   /* sigma_noise^2 */
    float delta;                    /* 1 / steps_ode */
    int32_t use_graph;
    int32_t reserved0;
    const uint8_t* host_cb_mask;    /* optional host [steps]: iterations after which iter_cb is called; NULL = every iteration */
} pf_ot_ode_params;
int pf_ot_ode_restore(pf_engine* e, const pf_degradation* d, const pf_ot_ode_params* prm, const float* y, float* x_inout, int B,
                      void* stream, void (*iter_cb)(int iteration, void* user), void* user);
/* Krylov iterations enqueued by the engine loop of the last pf_ot_ode_restore (0 when its operator has a closed-form solve) */
int64_t pf_ot_ode_krylov_iterations(const pf_engine* e);

/* ---- D-Flow (pnpflow/methods/d_flow.py) ------------------------------------------------------------------------------------
 * T(z) = steps_euler - 1 explicit midpoint steps of the velocity net (forward_flow_matching, d_flow.py:41-49):
 *   z += delta * v(z + delta/2 * v(z, t_i), t_i + delta/2),  t_i = delta * i + start_time,  delta = (1 - start_time) / (steps_euler - 1)
 * The schedule comes as host fp32 tables computed with the reference's own expressions; the net sees t * the solver time scale
 * (pf_engine_set_solver_time_scale: 999 for the NCSN++ net). */
typedef struct pf_d_flow_params {
    int32_t steps_euler;          /* >= 2 */
    int32_t use_graph;            /* capture the call into a hipGraph once and replay it while the arguments below stay the same */
    const float* host_t;          /* host [steps_euler - 1]: t_i */
    const float* host_t_mid;      /* host [steps_euler - 1]: t_i + delta/2 */
    float delta;                  /* fp32(delta) */
    float half_delta;             /* fp32(delta / 2) */
} pf_d_flow_params;
/* x_out = T(z); z, x_out: [B,C,H,W] */
int pf_d_flow_forward(pf_engine* e, const pf_d_flow_params* prm, const float* z, float* x_out, int B, void* stream);
/* One LBFGS closure of d_flow.py:110-121 at z, per image b:
 *   loss_per_image[b] = |H(T(z_b)) - y_b|^2 + lmbda (0.5 clamp(|z_b|^2, -1e6, 1e6) - (d-1) log(|z_b| + 1e-5)),  d = C*H*W
 *   grad = d sum_b loss_per_image[b] / dz   (the hand-written adjoint of T seeded with 2 H_adj(r), plus the regulariser gradient)
 * The ten evaluation inputs of T are kept; every VJP of the reverse sweep re-runs its forward under the retained plan.  Reductions are
 * deterministic (fp64 per-block partials, fixed-order finish).  Afterwards the retained forward (pf_unet_backward) is that of (z, t_0).
 * y: [B,C,Hy,Wy]; loss_per_image: device [B]; grad: [B,C,H,W].  The engine owns the operator scratch. */
int pf_d_flow_value_and_grad(pf_engine* e, const pf_degradation* d, const pf_d_flow_params* prm, const float* z, const float* y, float lmbda,
                             float* loss_per_image, float* grad, int B, void* stream);

/* Adaptive Dormand-Prince 5(4) solve of dx/dt = v(x, t) from t0 to t1 (torchdiffeq odeint(method='dopri5') as inverse_flow_matching,
 * d_flow.py:51-60, calls it with t 1 -> 0): RMS error norm over the whole batch tensor (one step sequence for all images), Hairer's
 * initial step, FSAL, 4th-order dense output at t1.  Step control runs on the host (one 8-byte read of the error ratio per attempt).
 * stats (host, may be NULL): [accepted steps, rejected steps, velocity evaluations].  More than max_steps attempts fails with
 * PF_ERR_NUMERIC and no result.  Synchronises `stream`. */
typedef struct pf_dopri5_params {
    double t0, t1;
    double rtol, atol;
    int32_t max_steps;
    int32_t reserved0;
} pf_dopri5_params;
int pf_flow_ode_dopri5(pf_engine* e, const pf_dopri5_params* prm, const float* x_in, float* x_out, int B, int64_t* stats, void* stream);

/* ---- the prior itself: Hutchinson divergence, sampling, log-likelihood -----------------------------------------------------------
 * Value of the Hutchinson-Skilling trace estimator (utils.hut_estimator, pnpflow/utils.py:243-270; get_div_fn,
 * image_generation/likelihood.py:27-38): div[b] = eps_b . (J_v(x, t) eps)_b = eps_b . (J_v(x, t)^T eps)_b - one retained forward at (x, t), one
 * hand-written backward with vec = eps, then a deterministic per-image dot product (fp64 per-block partials, fixed-order finish).  The
 * net sees t * the solver time scale.  A VALUE only: the gradient of the trace term with respect to x (what Flow-Priors differentiates,
 * hut_estimator(create_graph=True)) is a second-order pass the engine does not have; pf_flow_priors_grad obtains it from two of these
 * first-order VJPs instead.
 * t: device [B]; eps: [B,C,H,W]; v_out: [B,C,H,W] or NULL (the velocity v(x, t)); div_out: device double[B].  Afterwards the retained
 * forward (pf_unet_backward) is that of (x, t). */
int pf_flow_divergence(pf_engine* e, const float* x, const float* t, const float* eps, float* v_out, double* div_out, int B, void* stream);

/* torchdiffeq's fixed-grid `euler` over host_t[0 .. n_points - 1] (FLOW_MATCHING.generate_samples, pnpflow/train_flow_matching.py:170-198):
 *   x += (host_t[i+1] - host_t[i]) * v(x, host_t[i]),  the difference in fp32, a separate multiply and add.
 * Nothing synchronises inside the loop.  x_in, x_out: [B,C,H,W] (may alias); n_points >= 2. */
int pf_flow_ode_euler(pf_engine* e, const float* host_t, int n_points, const float* x_in, float* x_out, int B, void* stream);

/* The log-likelihood solve of get_likelihood_fn_rf (image_generation/likelihood.py:172-193): the augmented state (x, logp[B]) with
 *   dx/dt = v(x, t),  d logp_b/dt = eps_b . (J_v(x, t)^T eps)_b
 * from t0 to t1 under scipy.integrate.solve_ivp(method='RK45')'s rules (csrc/rk45_control.h): Dormand-Prince 5(4), the RMS error norm over
 * all B*C*H*W + B entries with scale atol + rtol max(|y|, |y_new|), SciPy's initial step, the last step clipped onto t1.  x is carried in
 * fp32, logp in fp64 on the device; time and step in fp64 on the host, the net is fed float(t) * the solver time scale.  Per attempt: six
 * VJP evaluations (FSAL) and one 8-byte read of the error norm.
 *   z_out: [B,C,H,W] the state at t1;  delta_logp: device double[B];  bpd: device float[B] or NULL,
 *   bpd[b] = -(-N/2 ln(2 pi) - 1/2 |z_b|^2 + delta_logp[b]) / (N ln 2) + offset,  N = C*H*W
 *   stats (host int64[3], may be NULL): accepted steps, rejected steps, evaluations (2 + 6 * attempts)
 * More than max_attempts attempts, a step below SciPy's min_step (10 ulp of t) or a non-finite error norm fail with PF_ERR_NUMERIC and no
 * result.  Afterwards the retained forward is that of the last evaluation.  Synchronises `stream`. */
typedef struct pf_likelihood_params {
    double t0, t1;
    double rtol, atol;
    double offset;
    int32_t max_attempts;
    int32_t reserved0;
} pf_likelihood_params;
int pf_flow_likelihood_rk45(pf_engine* e, const pf_likelihood_params* prm, const float* x_in, const float* eps, float* z_out, double* delta_logp,
                            float* bpd, int64_t* stats, int B, void* stream);

/* ---- sampling the rectified-flow prior (additive: PF_ABI_VERSION unchanged) -----------------------------------------------------------
 * euler_sampler of image_generation/sampling.py:69-109 (and RectifiedFlow.euler_ode, sde_lib.py:75-94, at sigma_var = 0), quirks kept.  For
 * i = 0 .. n_steps - 1, N = n_steps:
 *   num_t = i/N (t_end - t_begin) + t_begin,   dt = 1/N   (NOT the grid spacing (t_end - t_begin)/N: the reference's own step),
 *   sigma_t = (1 - num_t) sigma_var,   pred = v(x, num_t)   (the net is fed float(num_t) * the solver time scale),
 *   pred_sigma = pred + sigma_t^2 / (2 noise_scale^2 (1 - num_t)^2) (0.5 num_t (1 - num_t) pred - 0.5 (2 - num_t) x),
 *   x += pred_sigma dt + sigma_t sqrt(dt) n_i.
 * One fused kernel per step; the scalars are computed in double on the host and rounded to fp32 once each.  n_i = noise[i] when `noise`
 * (device [n_steps][B][C][H][W]) is given; otherwise it is drawn inside the kernel from Philox4x32-10/Box-Muller (seed, stream_id) at element
 * offset i * B*C*H*W: the values pf_fill_normal_at(out, B*C*H*W, seed, stream_id, i * B*C*H*W) writes.  sigma_var == 0: no noise is read or
 * drawn, the step is x + pred dt.  Nothing synchronises.  x_in, x_out: [B,C,H,W] (may alias).
 * PF_ERR_INVALID with nothing launched: a NULL engine, prm, x_in or x_out, B <= 0, n_steps < 1, sigma_var < 0, noise_scale <= 0, non-finite
 * or equal end points, and sigma_var > 0 with a step at num_t = 1. */
typedef struct pf_rf_sampler_params {
    double t_begin, t_end;    /* the reference: 1e-3, sde.T = 1 */
    int32_t n_steps;          /* sde.sample_N */
    int32_t reserved0;
    double sigma_var;         /* config.sampling.sigma_variance */
    double noise_scale;       /* config.sampling.init_noise_scale */
    uint64_t seed, stream_id; /* Philox key and stream of the in-kernel draw */
} pf_rf_sampler_params;
int pf_rf_euler_sampler(pf_engine* e, const pf_rf_sampler_params* prm, const float* x_in, const float* noise, float* x_out, int B, void* stream);

/* dx/dt = v(x, t) from t0 to t1 (either direction) under scipy.integrate.solve_ivp(method='RK45')'s rules (csrc/rk45_control.h), the solve
 * rk45_sampler (sampling.py:111-153) and RectifiedFlow.ode (sde_lib.py:37-72) make.  The state stays on the device in fp32; time and step in
 * fp64 on the host; the net is fed float(t) * the solver time scale.  The error norm is the RMS over ALL B*C*H*W entries with scale
 * atol + rtol max(|y|, |y_new|): SciPy sees the flattened batch as one vector, so the images of a batch share one step sequence (a sample
 * depends on its batch companions at the level of the tolerance).  Per attempt: six evaluations (FSAL) and one 8-byte read of the norm.
 *   stats (host int64[3], may be NULL): accepted steps, rejected steps, evaluations (2 + 6 * attempts)
 * More than max_attempts attempts, a step below 10 ulp of t or a non-finite norm fail with PF_ERR_NUMERIC and no result.  PF_ERR_INVALID with
 * nothing launched: a NULL engine, prm, x_in or x_out, B <= 0, rtol or atol <= 0, non-finite or equal end points, max_attempts <= 0.
 * Synchronises `stream`. */
typedef struct pf_rk45_params {
    double t0, t1;
    double rtol, atol;
    int32_t max_attempts;
    int32_t reserved0;
} pf_rk45_params;
int pf_flow_ode_rk45(pf_engine* e, const pf_rk45_params* prm, const float* x_in, float* x_out, int64_t* stats, int B, void* stream);

/* ---- whole restoration loop --------------------------------------------------------- */
typedef struct pf_pnp_params {
    int32_t steps;            /* steps_pnp */
    int32_t num_samples;
    const float* host_t;      /* host [steps]  : t value of each iteration (fp32, as the reference computes it) */
    const float* host_coef;   /* host [steps]  : lr_t / sigma^2 of each iteration */
    uint64_t seed;            /* Philox key for the interpolation noise */
    uint64_t stream_base;     /* noise stream id of (iteration it, sample s) = stream_base + it*num_samples + s */
    const float* noise;       /* optional device [steps*num_samples][B*C*H*W] injected noise (parity runs) */
    int32_t use_graph;        /* capture one outer iteration in a hipGraph and replay it */
    int32_t noise_model;      /* 0 gaussian (pf_grad_step), 1 laplace (pf_grad_step_laplace) */
    int32_t batch_samples;    /* evaluate the num_samples velocities of an iteration as one U-Net pass over num_samples*B images */
    int32_t reserved0;
    uint64_t elem_offset;     /* first normal number of this shard inside every (iteration, sample) noise stream: lo*C*H*W for the
                                 shard that owns images [lo, hi) of a global batch (0 for a single-device run); see pf_fill_normal_at */
    const uint8_t* host_cb_mask; /* optional host [steps]: iter_cb is called (stream synchronised) only after iterations with a non-zero
                                 entry - the reference's logging iterations, pnp_flow.py:128-139; NULL = after every iteration */
} pf_pnp_params;

/* Runs pnp_flow.py:93 and 102-121 for one batch:  x0 = H_adj(1);  `steps` iterations.
 * y: measurement [B,C,Hy,Wy]; x_out: [B,C,H,W].  iter_cb, if non-NULL, is called on the
 * host after each iteration (stream synchronised) - used for the periodic metrics. */
typedef void (*pf_iter_callback)(int iteration, void* user);
int pf_pnp_flow_restore(pf_engine* e, const pf_degradation* d, const pf_pnp_params* prm,
                        const float* y, float* x_out, int B, void* stream,
                        pf_iter_callback iter_cb, void* user);

/* ---- Prox-PnP with the gradient-step denoiser (pnpflow/methods/pnp_gs.py, pnpflow/train_denoiser.py) ---------------------------
 * The denoiser net is the same U-Net as the OT net (pnpflow/utils.py:170-180); the noise level sigma[B] is fed where the flow net takes t[B].
 *
 * GRADIENT_STEP_DENOISER.calculate_grad (train_denoiser.py:39-57):
 *   N = UNet(x, sigma),  Dg = (x - N) - J_N(x)^T (x - N),  g = 0.5 sum (x - N)^2 over the whole batch
 * sigma: device [B]; Dg, N: [B,C,H,W] (N may be NULL); g: device double[1] (may be NULL).  One retained forward and one backward;
 * afterwards the retained forward (pf_unet_backward) is that of (x, sigma). */
int pf_gs_denoiser_grad(pf_engine* e, const float* x, const float* sigma, float* Dg, float* N, double* g, int B, void* stream);

/* Iterations [first, stop) of PROX_PNP.solve_ip's loop (pnp_gs.py:132-222) for one batch, on the device:
 *   algo 0 (pgd, :202-222)                        z = x - lr grad_datafit(x) (skipped when skip_grad_step);  x = z - alpha Dg(z, level)
 *   algo 1 (hqs, random_inpainting, :138-156)     Dx = x - Dg(x, level);  x = H(y) - H(Dx) + Dx on every iteration but max_iter - 1, which
 *                                                 leaves x unchanged (its denoiser evaluation is skipped)
 *   algo 2 (hqs, gaussian_deblurring_FFT, :158-178)  y' = 0.1 alpha (x - Dg) + alpha (1 - 0.1 alpha) x;
 *                                                 x_new = real(ifft2(fft2(alpha H_adj(y) + y') / (alpha |fft2 filter|^2 + 1)));
 *                                                 alpha *= 0.9 when 0.5 |H(x_new) - y|^2 - 0.5 |H(x) - y|^2 < 0.1 / alpha |x_new - x|^2
 *                                                 (norms over the whole batch tensor)
 *   algo 3 (hqs, superresolution through a blur kernel; the schedule of :180-200)  z = 0.065 alpha (x - Dg) + alpha (1 - 0.065 alpha) x;
 *                                                 x_new = prox(z), the exact proximal map of alpha/2 |H x - y|^2 (pf_sr_prox with in = z + alpha H_adj(y));
 *                                                 alpha never decays and there is no gap log.  The reference's own prox_datafit for this branch
 *                                                 (pnp_gs.py:45-76) multiplies the aliased power spectrum by the data spectrum and is not a proximal map
 * The denoiser level of iteration i is host_sigma_den[i]; alpha lives in a device double (a decay needs no host round-trip).  One
 * iteration (retained forward, seed, hand-written backward, combine and, for algo 2, the Fourier prox, the reductions and the decision) is
 * captured once into a hipGraph and replayed while the plan, the operator, B, algo and the coefficients stay the same.  Reductions are
 * deterministic (fp64 per-block partials, fixed-order finish).  x_inout: the initialisation (or the iterate entering iteration `first`)
 * on entry, the iterate after iteration stop - 1 on exit.  host_alpha_out (host double[1], may be NULL): alpha after the call.
 * host_log (host double[2 * max_iter], may be NULL; algo 2): (gap, threshold) of every iteration run.  Afterwards the retained forward
 * is that of the last iteration's denoiser input.  Synchronises `stream` and checks the numeric health before returning.
 * PF_ERR_INVALID (no kernel launched): algo 1 without a PF_DEG_MASK_INPAINTING mask, algo 2 without PF_DEG_GAUSSIAN_BLUR, algo 3 without
 * PF_DEG_PSF_SR / PF_DEG_SR_FILTERED, laplace with algo != 0, first > stop or stop > max_iter. */
typedef struct pf_pnp_gs_params {
    int32_t algo;                 /* 0 pgd | 1 hqs random_inpainting | 2 hqs gaussian_deblurring_FFT | 3 hqs superresolution_blur / superresolution_bicubic */
    int32_t noise_model;          /* 0 gaussian | 1 laplace (pgd only) */
    int32_t max_iter, first, stop;
    int32_t skip_grad_step;       /* pgd, gaussian denoising (pnp_gs.py:204-210) */
    const float* host_sigma_den;  /* host [max_iter]: denoiser level of each iteration */
    float grad_coef;              /* lr / sigma^2 (gaussian) or lr / sigma (laplace) */
    int32_t use_graph;
    double alpha;                 /* on entry */
    const uint8_t* host_cb_mask;  /* as pf_pnp_params */
} pf_pnp_gs_params;
int pf_pnp_gs_restore(pf_engine* e, const pf_degradation* d, const pf_pnp_gs_params* prm, const float* y, float* x_inout, double* host_alpha_out,
                      double* host_log, int B, void* stream, pf_iter_callback iter_cb, void* user);

/* ---- Flow-Priors (pnpflow/methods/flow_priors.py) -----------------------------------------------------------------------------
 * Per outer iteration i of N: t = i/N (1 - eps0) + eps0 (eps0 = start_time, or 1e-3 with dt = 1/N when start_time <= 0), a fresh Adam
 * (lr = eta, betas (0.9, 0.999), eps 1e-8), K inner steps on
 *   loss(x) = lmbda |H(x + v(x, t) dt) - y_next|^2 (gaussian) | lmbda |.|_1 (laplace)  +  dt eps . J_v(x, t) eps  (+ 0.5 |x|^2 on iteration 0),
 *   y_next = (t + dt) y + (1 - (t + dt)) H(x_init),
 * the detached grad_xt_lik = -1/(1 - t) (-x + t v(x, t)) added to the gradient on every later iteration, then x += v(x, t) dt.
 * The gradient of the trace term is the central difference of two first-order VJPs (flow_priors.py differentiates hut_estimator's
 * jvp a second time):  dt (J(x + h eps)^T eps - J(x - h eps)^T eps) / (2 h),  h = fd_step;  O(h^2) truncation.  Per inner step: three retained
 * forwards and three backwards.  The net sees t * time_scale (999 for the NCSN++ net). */
typedef struct pf_flow_priors_params {
    int32_t N;                /* outer iterations (>= 1) */
    int32_t K;                /* Adam steps per outer iteration (>= 1) */
    int32_t first;            /* pf_flow_priors_restore runs outer iterations [first, stop) ... */
    int32_t stop;             /* ... 0 = N */
    double lmbda;
    double eta;               /* Adam's lr */
    double start_time;        /* < 1 */
    double fd_step;           /* h > 0 of the central difference */
    int32_t noise_model;      /* 0 gaussian | 1 laplace */
    int32_t reserved0;
    uint64_t seed;            /* Philox key of the engine's Rademacher probes (pf_fill_rademacher) */
    uint64_t stream_base;     /* probe of inner step k of outer iteration i: stream id stream_base + i * K + k, element offset 0 */
    double time_scale;        /* label = t * time_scale (> 0) */
} pf_flow_priors_params;

/* One Adam step of torch.optim.Adam's single-tensor form on device arrays of n values (any n, any alignment): step >= 1 is the
 * optimiser's step count after the update; the bias corrections are computed in double on the host (csrc/adam_step.h). */
int pf_adam_step(float* x, float* m, float* v, const float* g, int64_t n, double lr, double beta1, double beta2, double eps, int step, void* stream);

/* The gradient of one inner step of outer iteration `iteration` at x with the probe eps ([B,C,H,W], +-1), no update:
 *   out_g_data = w + dt J(x)^T w,  w = H_adj(2 lmbda r) | H_adj(lmbda sign r),  r = H(x + pred dt) - y_next
 *   out_g_trace = dt (J(x + h eps)^T eps - J(x - h eps)^T eps) / (2 h)
 *   out_g = out_g_data + out_g_trace + (x when iteration == 0, else grad_xt_lik);  out_pred = v(x, t)
 * Any of the four outputs may be NULL.  x, x_init: [B,C,H,W]; y: [B,C,Hy,Wy]. */
int pf_flow_priors_grad(pf_engine* e, const pf_degradation* d, const pf_flow_priors_params* prm, const float* x, const float* x_init, const float* y,
                        const float* eps, int iteration, float* out_g, float* out_g_data, float* out_g_trace, float* out_pred, int B, void* stream);

/* Outer iterations [first, stop) of the loop for one batch, on the device; no host synchronisation inside the loop.
 * x_inout: the result; with first > 0 also the iterate entering iteration `first` (with first == 0 the loop starts from x_init).
 * eps_or_null: (stop - first) * K injected probes [B,C,H,W] each, in the order they are used; NULL = the engine's Rademacher fill, numbered as
 * pf_flow_priors_params.stream_base says.  Synchronises `stream` and checks the numeric health before returning.
 * PF_ERR_INVALID with a pf_last_error text (nothing launched): N < 1, K < 1, fd_step <= 0, start_time >= 1, an unknown noise model,
 * a batch outside 1..65535 (no plan can be built for it), first / stop out of order. */
int pf_flow_priors_restore(pf_engine* e, const pf_degradation* d, const pf_flow_priors_params* prm, const float* y, const float* x_init,
                           const float* eps_or_null, float* x_inout, int B, void* stream);

/* Numeric health of the forwards run so far: every GroupNorm finalisation checks the activation statistics it consumes; an
 * overflow / NaN anywhere upstream makes them non-finite and sets a device flag.  This call synchronises `stream`, returns
 * PF_ERR_NUMERIC if the flag was set (and clears it), PF_OK otherwise.  pf_pnp_flow_restore checks it before returning.
 * (The reference computes in plain fp32, pnpflow/models.py:94-113; the split-fp16 operands of the default precision mode are
 * range-guarded by a per-image power-of-two scale, this is the loud backstop.) */
int pf_engine_check_numerics(pf_engine* e, void* stream);

/* device bytes currently held by the engine (weights, activation plans, solver buffers): what torch.cuda.max_memory_allocated
 * cannot see of the reference's `compute_memory` bookkeeping (pnpflow/methods/pnp_flow.py:99-100, 141-146). */
int64_t pf_engine_memory_bytes(const pf_engine* e);

/* kernel-time accounting for bench.py: enables HIP-event timing of the U-Net conv-GEMM
 * launches on `stream`; read back accumulated (count, milliseconds). */
int pf_engine_profile(pf_engine* e, int enable);
int pf_engine_profile_read(pf_engine* e, int64_t* launches, double* ms_conv_gemm, double* flops_conv_gemm);

#ifdef __cplusplus
}
#endif
#endif /* PNPFLOW_HIP_H */
