/*
 * uwie.h -- C ABI of libuwie.so: the MI355X (gfx950) implementation of the
 * underwater-image-enhancement hot path.
 *
 * The reference (submarine0418/underwater_image_enhancement) is pure Python and
 * has NO FFI/plugin interface for this path; the entry points below are what a
 * ctypes binding for it would call.  Each one names the reference interface it
 * replaces (S6 = six_stadigy.py, ES = enhancement_strategies.py).
 *
 * Conventions
 *   - every pointer named d_* is a DEVICE pointer (HBM); images are HWC,
 *     RGB-interleaved, contiguous, batch-major: [batch][H][W][3];
 *   - every call enqueues work on `stream` (a hipStream_t passed as void*) and
 *     returns without synchronising; scalars that the reference reads back on
 *     the host (cast kind, atmospheric light, percentiles) stay on the device;
 *   - the library never allocates or frees caller memory: scratch comes from
 *     the caller (`d_workspace`, sized by uwie_workspace_bytes);
 *   - return value: 0 on success, a negative UWIE_E_* code on failure; the
 *     message is available from uwie_last_error() (thread-local);
 *   - a context belongs to one device and one host thread/stream at a time.
 */
#ifndef UWIE_H_
#define UWIE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UWIE_OK 0
#define UWIE_E_INVALID (-1)   /* bad argument (null pointer, size, unknown strategy: ES:500-501 ValueError) */
#define UWIE_E_WORKSPACE (-2) /* workspace too small */
#define UWIE_E_HIP (-3)       /* a HIP runtime call failed */
#define UWIE_E_NODEVICE (-4)  /* no gfx950 device / code object cannot load */
#define UWIE_E_DEVICE (-5)    /* a kernel found one of its own invariants violated (uwie_device_status) */

/* which reference surface's arithmetic to follow */
#define UWIE_SURFACE_SIX 0  /* six_stadigy.EnhancementStrategies.strategy1..6 (S6:230-285)        */
#define UWIE_SURFACE_DICT 1 /* enhancement_strategies.EnhancementStrategies.apply_strategy (ES:477) */

/* strategy ids.  SIX: 1..6 as in S6:230-285.  DICT: the keys of ES:489-498. */
#define UWIE_DICT_STRONG_DEHAZING 0
#define UWIE_DICT_MEDIUM_DEHAZING 1
#define UWIE_DICT_LIGHT_ENHANCEMENT 2
#define UWIE_DICT_CLAHE_ENHANCEMENT 3
#define UWIE_DICT_HISTOGRAM_EQUALIZATION 4

#define UWIE_CAST_NORMAL 0
#define UWIE_CAST_GREENISH 1
#define UWIE_CAST_BLUISH 2

typedef struct uwie_ctx uwie_ctx;

/* Numeric parameters of one strategy.  uwie_params_init fills the reference's
 * hard-coded (SIX, S6:230-285) or in-code default (DICT, ES:356-372,382-395,
 * 405-419,428-441,466-473) values; the host wrapper overrides fields from the
 * caller's params dict (config.py:28-75 value sets). */
typedef struct uwie_params {
    int32_t surface;       /* UWIE_SURFACE_*                                                     */
    int32_t strategy;      /* see above                                                          */
    int32_t cast_correct;  /* 1: detect_image_type + color_correction first (S6:409,413)         */
    int32_t forced_cast;   /* -1: detect (if cast_correct).  UWIE_CAST_*: skip detection and apply
                              color_correction for this kind (caller ran detect_image_type itself)  */
    int32_t gray_shift;    /* RGB2GRAY fixed point: 15 (OpenCV 4.x, default) or 14               */
    int32_t min_size;      /* quadtree leaf size (S6:49, ES:77): 1                               */
    double omega;          /* S6:173 / ES:225 (a Python float there: float32 arithmetic rounds it, float64 keeps it) */
    int32_t gf_ksize;      /* guided-filter box WIDTH `r` (S6:31, ES:31)                         */
    double gf_eps;         /* S6: 0.5/0.5/0.1 (:234,245,255); ES: always 0.001 (:209)            */
    double L_low, L_high;  /* percentile stretch bounds in percent (S6:191, ES:252)              */
    double wb_percentile;  /* S6:211 white_balance percentile; < 0 = stage absent                */
    double clip_limit;     /* CLAHE clip limit (S6:202, ES:288); <= 0 = stage absent             */
    int32_t tiles_x, tiles_y; /* CLAHE tile grid (S6: 8x8 fixed; ES: tile_grid_size)             */
    double gamma;          /* S6:222 exponent g (x**g); ES:276 g (clip(x**(1/g)))                */
    int32_t apply_gamma;   /* 0/1 (ES `apply_gamma`; S6 strategies 1,4,5,6 always 1)             */
    int32_t gf_exact;      /* guided filter: 1 = reproduce cv2.boxFilter's float64 running-sum order bit for
                              bit (6 materialised planes); 0 (default) = fused single-kernel float64 filter,
                              same window/border, free summation order: |t - t_exact| <= 1e-11 (observed 7e-15).
                              What that means for the u8 OUTPUT of gf_exact = 0: the same bytes as gf_exact = 1 except
                              where the exact value of a pixel sits on a truncation boundary ahead of CLAHE, so that the
                              last bit of t decides its byte -- about one pixel in 1e9 bytes (two in a 25 440-case soak,
                              profiles/r03_soak.txt; tests/test_gpu_fuzz.py keeps one such frame) -- and that pixel then
                              differs by up to CLAHE's local slope (<= clip_limit) times gamma's slope: 2 - 3 LSB seen,
                              1 LSB without CLAHE.  gf_exact = 1 has no such pixel; it costs ~6x the filter's time.
                              The DICT surface's float64 image differs in its last bits (<= 1e-11) under gf_exact = 0. */
    int32_t inter_dtype;   /* number format of the guided filter's a/b intermediates (S6:39-43) when gf_exact = 0:
                              UWIE_INTER_F64 (default) float64 like the reference; UWIE_INTER_FX32 32-bit fixed
                              point (BASELINE.json configs[4] "reduced-precision intermediates": a and b are rounded
                              once to 2^-31 / 2^-30, every sum stays exact; |t - t_exact| <= 5e-10; u8 output: about
                              one byte in 1e6-1e7 differs, by 1 LSB before CLAHE and up to CLAHE's local slope
                              after it -- tests/test_gpu_fuzz.py).  SIX surface only (needs the pre-clipped transmission, S6:174); other
                              cases silently keep float64.
                              UWIE_INTER_F32T (round 3; BASELINE.json configs[4] "fp16 intermediates ... stated tolerance"):
                              the refined transmission (S6:180) is stored as float32 and restore_image (S6:183-188) runs in
                              float32 with a reciprocal instead of the float64 division: half the bytes of the t plane, a
                              quarter of the restore arithmetic.  NOT the <= 1 LSB mode -- its own contract against the float64
                              path: >= 99.98 % of the u8 bytes identical, <= 5e-5 of them off by more than 1 LSB, none by more
                              than 10, PSNR >= 80 dB (tests/test_gpu_fuzz.py::test_f32t_transmission_stated_tolerance).  SIX
                              surface, strategies 1-3, windows 10 / 15 / 20 on frames the wavefront kernels take (even W,
                              H >= 4k, W >= 2k); everything else silently keeps float64.                         */
    int32_t dark_patch;    /* side k of the square patch the dark channel is taken over (He et al.'s dark channel prior uses
                              15).  1 (default; 0 means 1, so a zero-filled struct keeps it) is the reference: the minimum
                              over the three channels of ONE pixel (S6:170-171, ES:221-222).  dark_patch > 1 HAS NO REFERENCE
                              COUNTERPART; its contract is this definition.  For an H x W plane d, k >= 1 and the anchor
                              a = k / 2 (integer division),
                                erode(d)[y, x] = min{ d[v, u] : y - a <= v <= y + k - 1 - a,  x - a <= u <= x + k - 1 - a,
                                                               (v, u) inside the image }
                              which is cv2.erode with a k x k rectangle, its default centre anchor and its default border:
                              pixels outside the frame never win.  Even k is allowed and asymmetric as written (k = 4 covers
                              x - 2 .. x + 1).  The transmission is the surface's own arithmetic with erode between the channel
                              minimum and 1 - omega * dark: float32, eps = 1e-6 and the clip to [0.1, 1] on the SIX surface
                              (S6:170-174), eps = 1e-10 and no clip on the DICT surface (ES:221-225).  The guide image, the
                              atmospheric light, the restore step and everything after them read the original frame.
                              Valid: 0 .. 31.  u8 frames only: uwie_enhance_f32 / _f64 return UWIE_E_INVALID for > 1.
                              A patched call writes the t0 plane first (k_trans_patch) and never takes the route that
                              evaluates t0 inside the guided filter (tuning gf_fuse).                              */
} uwie_params;

#define UWIE_INTER_F64 0
#define UWIE_INTER_FX32 1
#define UWIE_INTER_F32T 2

const char *uwie_last_error(void);
const char *uwie_version(void);

int uwie_create(int device, uwie_ctx **out_ctx);
void uwie_destroy(uwie_ctx *ctx);

/* Device-side self checks (no reference counterpart).  Kernels that chase indices through workspace memory validate every
 * index before dereferencing it; one that is out of range is not followed -- the kernel sets a bit in the context's
 * device status word and carries on with a safe substitute, so a defect in the library is an error code, never a memory
 * access fault.  Entry points do not synchronise, so they cannot report it themselves: uwie_device_status waits for
 * `stream`, returns UWIE_OK when no bit is set and UWIE_E_DEVICE otherwise (*bits, optional, receives the word; the word
 * is cleared).  A caller that reads results back synchronises anyway and calls this right after (the Python wrapper does).
 *   UWIE_STATUS_CANNY_LABEL  cv2.Canny's hysteresis (S6:150; k_canny.hip union / mark / emit / paint) met a component
 *                            label that the current launch did not write. */
#define UWIE_STATUS_CANNY_LABEL 1u
/*   UWIE_STATUS_FALLBACK_SYNC  reserved, never set (it reported a wait between the blocks of an earlier percentile fallback;
 *                              the selection's blocks no longer wait for each other). */
#define UWIE_STATUS_FALLBACK_SYNC 2u
/*   UWIE_STATUS_QTREE_BOUNDS   (tuning q_hist = 3 only: a checking route) a quadrant's reference-order score (compute_Q, S6:116-157)
 *                              fell outside the interval derived from its byte histogram, or the histogram route's decision
 *                              differs from the reference-order argmax: the rounding bounds of k_q_decide / k_q_tail are too tight. */
#define UWIE_STATUS_QTREE_BOUNDS 4u
/*   UWIE_STATUS_FEATURE_COUNTS  uwie_feature_extractor_u8 (k_extractor.hip k_fx_finish): the gray or the LBP histogram of a frame
 *                               does not hold every pixel once: that frame's features are not valid. */
#define UWIE_STATUS_FEATURE_COUNTS 8u
/*   UWIE_STATUS_DIFF_RANK  uwie_diff_gated_f32 / _save_f32 (k_select.hip k_sel_init_gated_ranks): an image's L_low or L_high gives
 *                          no valid sorted position by Python's rules (int(L / 100.0 * n) outside [-n, n - 1]: IndexError;
 *                          L NaN: ValueError; L infinite: OverflowError).  That image's output and gradients are NaN. */
#define UWIE_STATUS_DIFF_RANK 16u
/*   UWIE_STATUS_RESIZE_DESC  uwie_resize_rgb_u8 (k_resize.hip): a frame descriptor has a NULL pointer or a side outside
 *                            [1, UWIE_RESIZE_MAX_SRC]: nothing of that frame was read or written. */
#define UWIE_STATUS_RESIZE_DESC 32u
/*   UWIE_STATUS_CLASSIFY_NAN  uwie_classify_f64 / uwie_predict_strategy_u8 (k_classify.hip): a row holds NaN after scaling and
 *                             the model is GB or SVC (scikit-learn raises "Input X contains NaN"): that row's label is -1,
 *                             its proba NaN.  (Random forests route NaN and never set it.) */
#define UWIE_STATUS_CLASSIFY_NAN 64u
int uwie_device_status(uwie_ctx *ctx, void *stream, uint32_t *bits);

/* Per-kernel timing for benchmarks (no reference counterpart; the reference only has a per-image wall clock,
 * S6:393-500).  enable(1) starts recording one HIP-event pair per kernel launch on the launch stream;
 * collect() synchronises the device, folds the intervals by kernel name and returns the number of rows
 * (negative on error); row(i) reads one row.  Recording is per host thread. */
int uwie_profile_enable(uwie_ctx *ctx, int on);
/* Restrict recording to launches of one kernel (name as uwie_profile_row reports it); NULL or "" records all.  An event
 * pair per launch costs ~9 us of stream time, 6 % of a 4K x 64 step with every launch recorded: a benchmark that reports
 * whole-job time records the one kernel it needs. */
int uwie_profile_filter(uwie_ctx *ctx, const char *kernel_name);
int uwie_profile_collect(uwie_ctx *ctx);
int uwie_profile_row(uwie_ctx *ctx, int i, const char **name, double *total_ms, int *calls);

/* Fill `p` with the reference defaults for (surface, strategy). */
int uwie_params_init(uwie_params *p, int surface, int strategy);

/* Route selectors of a context: which of several equivalent routes a stage takes where uwie_params has no say (the parity
 * tests force the fallback routes this way, profiles/ scripts compare them).  Two classes:
 *   SAME BYTES on every setting -- the selection, storage and quadtree routes: select_generic (0), restore_store (0),
 *     lin_predict3 (0), lin_cap (0 = default), lin_no_predict (0), lin_predict_shift (0), rank_sweep (1: strategies 1-2 count
 *     ranks against the predicted windows; 0: the histogram sweep), q_hist (1: quadtree levels decided from byte histograms where
 *     the score intervals allow; 0: NumPy-order kernels only; 2: histograms taken, never used; 3: both, and every reference-order
 *     score is checked against its interval -- UWIE_STATUS_QTREE_BOUNDS), canny_prepass (1),
 *     streams (1; 2 .. 4 = sub-batches on internal streams), gf_fuse (2: the transmission's first half is evaluated inside the
 *     guided filter for window 15 (k_guided_split8, same float32 operations, no t0 plane) on jobs that fill the device: strips x bands
 *     x batch (uwie_guided_fill) at least one round of its compute units x 8; 1: whenever the split plan exists; 0: never,
 *     k_trans_init writes a t0 plane first),
 *     entry_fuse (1, round 4; SIX surface with cast detection, strategies 1-3, frames whose width is a multiple of 8: the
 *     level-0 quadrant histograms of estimate_atmospheric_light (S6:49-157) are counted by detect_image_type's own pass over
 *     the frame (S6:292) and that pass writes the gray plane (S6:149,177) for a cast kind guessed from 2048 pixels -- frames
 *     whose decision differs get their plane again; 2: histograms from that pass, the gray plane from the quadtree's level-0
 *     Canny pre-pass; 0: one pass over the frame per stage, as in rounds 1-3);
 *   SAME TRANSMISSION TO 1e-11, hence the u8 contract of uwie_params.gf_exact = 0 -- which fused guided-filter kernel runs:
 *     gf_split (1), gf_bands (0 = chosen from the job).  They sum the same windows in different orders.
 *   canny_fault_inject (0) is for tests/test_gpu_robustness.py only (it breaks an invariant on purpose; see uwie_device_status).
 * An environment variable UWIE_<NAME> sets the initial value; it is read once, in uwie_create -- no entry point reads the
 * environment.  Unknown names are an error. */
int uwie_set_tuning(uwie_ctx *ctx, const char *name, int value);
int uwie_get_tuning(uwie_ctx *ctx, const char *name, int *value);

/* Scratch bytes needed by uwie_enhance_u8 / any stage entry point for this shape, for a context with the DEFAULT route
 * selectors (p = NULL: any call).  uwie_workspace_bytes_ctx answers for a given context: the tuning selectors restore_store and
 * select_generic make the dehazing strategies keep the restored image in float32 planes (12 B/px more). */
size_t uwie_workspace_bytes(int batch, int H, int W, const uwie_params *p);
size_t uwie_workspace_bytes_ctx(uwie_ctx *ctx, int batch, int H, int W, const uwie_params *p);

/*
 * enhance(u8 RGB) -> u8 RGB for a whole batch.
 *   SIX : x = u8/255 (S6:406) -> [detect_image_type, color_correction (S6:409,413)]
 *         -> strategyN (S6:230-285) -> (y*255).astype(uint8) (S6:430)
 *   DICT: x = u8/255 (main.py:108) -> apply_strategy body (ES:350-474) -> (y*255).astype(uint8) (main.py:155)
 * d_out_f32 (optional, may be NULL) receives the float image the reference's
 * strategy function returns ([batch][H][W][3] float32; float64 values of the
 * DICT surface are rounded to float32).
 */
int uwie_enhance_u8(uwie_ctx *ctx, const uint8_t *d_in, uint8_t *d_out_u8, float *d_out_f32, int batch, int H, int W,
                    const uwie_params *p, void *d_workspace, size_t workspace_bytes, void *stream);

/* The dict surface with the reference's own result type: recover_image / clahe_enhancement / histogram_equalization /
 * color_enhancement / gamma_correction return float64 (ES:247,307,345,269-270,284-285), and the caller quantises THAT
 * ((enhanced * 255).astype(np.uint8), main.py:155).  d_out_f64: [batch][H][W][3] float64; d_out_u8 (optional) the device's
 * own quantisation of the same values.  UWIE_SURFACE_DICT only; same workspace as uwie_enhance_u8. */
int uwie_enhance_u8_f64(uwie_ctx *ctx, const uint8_t *d_in, uint8_t *d_out_u8, double *d_out_f64, int batch, int H, int W,
                        const uwie_params *p, void *d_workspace, size_t workspace_bytes, void *stream);

/* Read-only: the percentiles the last uwie_enhance_u8 / uwie_enhance_u8_f64 call on this workspace (same batch, H, W, p)
 * stretched with, widened to double, into d_out: [batch][3][2] (L_low, L_high) for SIX strategies 1-2 and the DICT
 * dehazing strategies, [batch][3][4] (lo1, hi1, lo2, hi2: the contrast stretch's and white balance's) for SIX strategy 3.
 * The buffers are found by the enhance call's own carving, sub-batch slices of tuning `streams` included, for the
 * context's CURRENT tuning: call it under the tuning of the enhance call.  The context remembers whether its last enhance
 * call was uwie_enhance_u8_f64, which never splits the batch, and reads that call's single layout then.  Dehazing
 * strategies only. */
int uwie_enhance_percentiles(uwie_ctx *ctx, const void *d_workspace, size_t workspace_bytes, int batch, int H, int W,
                             const uwie_params *p, double *d_out, void *stream);

/* The same strategies on GENERAL float images: the reference's functions take "float HxWx3 in [0, 1]" (S6:230-285,
 * ES:477-508) and its own harnesses feed np.random.rand (ES:516, example_usage.py:27,44,112).  uwie_enhance_u8 starts from
 * the u8 frame a float image was made of (the fast path: every kernel exploits that a pixel value is a function of its
 * byte); an image that is NOT u8-derived goes through these entry points: the same arithmetic with the pixel values read
 * from the float image, then the materialised-image stage kernels.  Written for parity, not speed.
 *   uwie_enhance_f32: float32 [batch][H][W][3] in.  SIX surface: strategy1..6(img) [with detect_image_type /
 *     color_correction first when cast_correct or forced_cast say so]; float32 image to d_out_f32, its (y*255).astype(u8)
 *     to d_out_u8.  DICT surface: apply_strategy body; the reference's float64 image to d_out_f64 (and/or float32 / u8).
 *   uwie_enhance_f64: float64 in, DICT surface only (six_stadigy.py works on float32 frames, S6:406).
 *   uwie_workspace_bytes_float: scratch bytes of either (elem_bytes = 4 or 8).
 *   uwie_cast_classify_f32: detect_image_type (S6:292-302) on a general float32 image. */
size_t uwie_workspace_bytes_float(int batch, int H, int W, const uwie_params *p, int elem_bytes);
int uwie_enhance_f32(uwie_ctx *ctx, const float *d_img, uint8_t *d_out_u8, float *d_out_f32, double *d_out_f64, int batch, int H, int W,
                     const uwie_params *p, void *d_workspace, size_t workspace_bytes, void *stream);
int uwie_enhance_f64(uwie_ctx *ctx, const double *d_img, uint8_t *d_out_u8, double *d_out_f64, int batch, int H, int W,
                     const uwie_params *p, void *d_workspace, size_t workspace_bytes, void *stream);
int uwie_cast_classify_f32(uwie_ctx *ctx, const float *d_img, int batch, int H, int W, int32_t *d_kind, float *d_mean_rgb, void *stream);
/* color_correction (S6:305-323) of a general float32 image: d_kind[b] = UWIE_CAST_* per image (NORMAL copies). */
int uwie_color_correct_f32(uwie_ctx *ctx, const float *d_img, const int32_t *d_kind, float *d_out, int batch, int H, int W, void *stream);

/* Scratch bytes uwie_enhance_all_u8 needs for these six parameter sets (NULL = the defaults): one layout sized for the
 * most demanding of them (exact-order guided filter planes, widest CLAHE tile grid). */
size_t uwie_workspace_bytes_all(int batch, int H, int W, const uwie_params *p6);

/*
 * The batch driver's inner loop (six_stadigy.py:398-431): one cast detection / correction per image, then all six
 * strategies on the corrected image.  The gray plane and the atmospheric light depend on the corrected image only, so
 * strategies 1-3 share one quadtree instead of running three (the reference recomputes it, with the same result).
 * d_out_u8 is [6][batch][H][W][3]: plane k holds strategy k+1.  d_kind (optional) receives UWIE_CAST_* per image
 * (the driver's image_type column).  p6: six parameter sets, strategies 1..6 in order, or NULL for the reference defaults.
 * Workspace: uwie_workspace_bytes(batch, H, W, <a strategy 1-3 parameter set>).
 */
int uwie_enhance_all_u8(uwie_ctx *ctx, const uint8_t *d_in, uint8_t *d_out_u8, int32_t *d_kind, int batch, int H, int W,
                        const uwie_params *p6, void *d_workspace, size_t workspace_bytes, void *stream);

/*
 * DifferentiableEnhancement.forward (vgg_16_UIE.py:32-128), the arithmetic behind
 * EnhancementPredictor.enhance_image (use_trained_model.py:83-111): per channel stretch between the sorted
 * positions int(L_low/100*n) and int(L_high/100*n) (torch.sort) -> [UWIE_DIFF_OMEGA] dark-channel dehazing with
 * A = 0.6 -> [UWIE_DIFF_GAMMA] pow(x + 1e-8, gamma) -> clamp(0, 1).  float32 in, float32 out, same layout:
 * planar != 0: [batch][3][H][W] (the module's NCHW), else [batch][H][W][3].
 * d_params: [batch][4] float32 = {L_low, L_high, omega, gamma} (the module's (B,1) parameter tensors).
 * Bit-exact against torch on the CPU except pow (<= 1 float32 ulp).  Workspace: uwie_workspace_bytes.
 */
#define UWIE_DIFF_OMEGA 1
#define UWIE_DIFF_GAMMA 2
int uwie_diff_enhance_f32(uwie_ctx *ctx, const float *d_img, float *d_out, int batch, int H, int W, int planar,
                          const float *d_params, int flags, void *d_workspace, size_t workspace_bytes, void *stream);

/*
 * Its gradient (vgg_16_UIE.DifferentiableEnhancement under torch autograd; the contract: DESIGN.md section 8).
 *   uwie_diff_enhance_save_f32: uwie_diff_enhance_f32 (the same output bytes, the same workspace) that also writes
 *     d_saved [batch][3][2] float32 = {p_lo, p_hi} of every plane, the two sorted values the stretch used.
 *   uwie_diff_enhance_bwd_f32: given the forward's inputs (d_img, d_params, flags, planar), its d_saved and
 *     d_grad_out = dL/d(out) in the image's layout, writes
 *       d_grad_img (NULL: skipped, parameter gradients only) = dL/d(img), same layout; the gradient of p_lo / p_hi
 *         goes to the element torch's stable CPU sort took it from;
 *       d_grad_params [batch][4] float32 = {0, 0, dL/d(omega), dL/d(gamma)} (L_low / L_high get no gradient: the
 *         reference reads them with .item()).
 *     Sums over pixels are float64 in a fixed order, without atomics: the same inputs give the same bits on every run.
 *     Two kernel launches.  Reads nothing the forward left in the workspace.  Workspace:
 *     uwie_diff_enhance_bwd_workspace_bytes(batch, H, W) (about 112 bytes per 2048 pixels, at most 57 KB per image).
 */
int uwie_diff_enhance_save_f32(uwie_ctx *ctx, const float *d_img, float *d_out, int batch, int H, int W, int planar,
                               const float *d_params, int flags, float *d_saved, void *d_workspace, size_t workspace_bytes,
                               void *stream);
size_t uwie_diff_enhance_bwd_workspace_bytes(int batch, int H, int W);
int uwie_diff_enhance_bwd_f32(uwie_ctx *ctx, const float *d_img, const float *d_params, int flags, int planar, int batch,
                              int H, int W, const float *d_saved, const float *d_grad_out, float *d_grad_img,
                              float *d_grad_params, void *d_workspace, size_t workspace_bytes, void *stream);

/*
 * The same module for u8 frames, in the byte domain (k_diff_u8.hip): what
 * EnhancementPredictor.process_single_image does from a decoded frame to a u8 frame (use_trained_model.py:113-164).
 * d_in: [batch][H][W][3] uint8, the frame whose float image is u8 / 255.  x = (float)v / 255.0f is strictly increasing in
 * the byte v, so the two sorted positions are two bins of the channel's 256-bin histogram and the stretch takes at most
 * 256 values per channel: two passes over the frame's bytes (count, apply), no float image anywhere.
 *   d_out_u8  [batch][H][W][3] uint8   = (uint8)(v * 255.0f) of the module's clamped output v (it holds no NaN: the final
 *             clamp turns NaN into 0), the bytes of (np.clip(enhanced, 0, 1) * 255).astype(np.uint8)
 *   d_out_f32 [batch][H][W][3] float32 = v, the bits uwie_diff_enhance_f32 gives for uwie_u8_to_f32 of the frame
 *   Either may be NULL, not both (UWIE_E_INVALID).  d_saved (optional): as uwie_diff_enhance_save_f32 leaves it.
 * d_in must be 4-byte aligned (UWIE_E_INVALID otherwise: the count pass reads dwords); the outputs need no alignment beyond
 * their element types.  Every check runs before the first launch.
 * Workspace: uwie_workspace_bytes_diff_u8(batch, H, W) = the histograms and the order statistics, about 3 KB per image
 * whatever H x W is (0: batch/H/W out of range).
 */
size_t uwie_workspace_bytes_diff_u8(int batch, int H, int W);
int uwie_diff_enhance_u8(uwie_ctx *ctx, const uint8_t *d_in, uint8_t *d_out_u8, float *d_out_f32, int batch, int H, int W,
                         const float *d_params /* [batch][4] L_low, L_high, omega, gamma */,
                         int flags /* UWIE_DIFF_OMEGA | UWIE_DIFF_GAMMA */, float *d_saved /* optional */, void *d_workspace,
                         size_t workspace_bytes, void *stream);

/*
 * deep_learning_parameters.DifferentiableEnhancement (deep_learning_parameters.py:24-90), the module EndToEndTrainer trains
 * through (the contract: DESIGN.md section 10).  Per plane: stretch between the sorted positions k = int(L_low / 100.0 * n)
 * and int(L_high / 100.0 * n) with Python's indexing rules (no clamp: a negative k counts from the end; an image whose k is
 * outside [-n, n - 1] or whose L is not finite sets UWIE_STATUS_DIFF_RANK and gets NaN) -> e = 1.0 / gamma (float32,
 * correctly rounded) -> z = pow(s + 1e-8, e) -> clamp(use_gamma * z + (1 - use_gamma) * s, 0, 1).
 * d_params: [batch][4] float32 = {L_low, L_high, use_gamma, gamma}; flags: reserved, 0.  Other arguments, layouts, d_saved
 * and the workspaces are those of the uwie_diff_enhance_* family above (forward workspace: uwie_workspace_bytes).
 *   uwie_diff_gated_bwd_f32: d_grad_params [batch][4] = {0, 0, dL/d(use_gamma), dL/d(gamma)}; d_grad_img optional (NULL:
 *     skipped); the same fixed-order float64 sums and stable-sort scatter, two kernel launches.
 * Bit-exact against torch on the CPU except pow (<= 1 float32 ulp; with use_gamma == 0 the output is exact).
 */
int uwie_diff_gated_f32(uwie_ctx *ctx, const float *d_img, float *d_out, int batch, int H, int W, int planar,
                        const float *d_params, int flags, void *d_workspace, size_t workspace_bytes, void *stream);
int uwie_diff_gated_save_f32(uwie_ctx *ctx, const float *d_img, float *d_out, int batch, int H, int W, int planar,
                             const float *d_params, int flags, float *d_saved, void *d_workspace, size_t workspace_bytes,
                             void *stream);
size_t uwie_diff_gated_bwd_workspace_bytes(int batch, int H, int W);
int uwie_diff_gated_bwd_f32(uwie_ctx *ctx, const float *d_img, const float *d_params, int flags, int planar, int batch, int H,
                            int W, const float *d_saved, const float *d_grad_out, float *d_grad_img, float *d_grad_params,
                            void *d_workspace, size_t workspace_bytes, void *stream);

/*
 * The gated module for u8 frames, in the byte domain (k_diff_u8.hip): the inference route of
 * EndToEndTrainer's stack from a decoded frame to a u8 frame.  d_in: [batch][H][W][3] uint8, the frame whose float image is
 * u8 / 255.  Nothing after the stretch mixes channels, so per image and channel the module is a function of the byte alone:
 * count (256 bins per channel), one block per image that finds the two sorted positions (Python's indexing rules, as above)
 * and tabulates the module for the 3 x 256 byte values, then a pure lookup over the frame's bytes.
 *   d_out_u8  [batch][H][W][3] uint8   = (uint8)(v * 255.0f) of the module's output v
 *   d_out_f32 [batch][H][W][3] float32 = v, the bits uwie_diff_gated_f32 gives for uwie_u8_to_f32 of the frame
 *   Either may be NULL, not both (UWIE_E_INVALID).  d_saved (optional): as uwie_diff_gated_save_f32 leaves it.
 * An image without a valid sorted position sets UWIE_STATUS_DIFF_RANK; its floats are NaN and its bytes 0, the other images
 * of the batch are not affected.  d_params: [batch][4] float32 = {L_low, L_high, use_gamma, gamma}; flags: reserved, 0.
 * d_in must be 4-byte aligned (UWIE_E_INVALID otherwise); the outputs need no alignment beyond their element types.  Every
 * argument check runs before the context is touched.
 * Workspace: uwie_workspace_bytes_diff_gated_u8(batch) = the histograms and the tables, 7 KB per image whatever H x W is
 * (0: batch < 1).
 */
size_t uwie_workspace_bytes_diff_gated_u8(int batch);
int uwie_diff_gated_u8(uwie_ctx *ctx, const uint8_t *d_in, uint8_t *d_out_u8, float *d_out_f32, int batch, int H, int W,
                       const float *d_params /* [batch][4] L_low, L_high, use_gamma, gamma */, int flags /* 0 */,
                       float *d_saved /* optional */, void *d_workspace, size_t workspace_bytes, void *stream);

/*
 * ReferenceLoss (deep_learning_parameters.py:170-196) and the L1 / MSE terms of CombinedLoss (vgg_16_UIE.py:272-303) on a
 * module's output o and a reference r (the contract: DESIGN.md section 13): d_loss [2] float32 = {l1, l2} =
 * {mean|o - r|, mean((o - r)^2)} over all N = batch * 3 * H * W values (torch's 'mean' reduction).  The float32 terms are
 * summed in float64 in a fixed order, without atomics, and rounded once: the same inputs give the same bits on every run.
 * The caller forms w1 * l1 + w2 * l2 on the device.  map:
 *   UWIE_LOSS_IDENTITY  o = d_img, any layout; d_params, flags, d_out and d_saved are not read (NULL).
 *   UWIE_LOSS_VGG       o = uwie_diff_enhance_f32 of (d_img, d_params, flags): d_out (NULL: not written) gets its bytes,
 *                       d_saved (required) what uwie_diff_enhance_save_f32 leaves there.
 *   UWIE_LOSS_GATED     o = uwie_diff_gated_f32 of (d_img, d_params), the same way (flags: 0).  An image without a valid
 *                       sorted position sets UWIE_STATUS_DIFF_RANK and makes both values NaN.
 * d_ref: float32 in d_img's layout.  Workspace: uwie_ref_loss_workspace_bytes(batch, H, W).
 *   uwie_ref_loss_bwd_f32: the gradient of g1 * l1 + g2 * l2 (+ <d_grad_out, o>), with d_grad_loss [2] = {g1, g2} read on the
 *     device (no host sync).  dL/do follows torch's autograd formulas in their order (MeanBackward0 -> AbsBackward0 with
 *     sgn(0) = 0, MseLossBackward0, their sum, then d_grad_out when given), then the module's backward exactly as
 *     uwie_diff_enhance_bwd_f32 / uwie_diff_gated_bwd_f32 with that gradient as grad_out.  The same arguments as the forward
 *     (d_saved: the forward's); identity: d_grad_img (required) = dL/do; otherwise d_grad_img (NULL: skipped) and
 *     d_grad_params (required) as in those entry points.  d_grad_img must not alias d_img, d_ref or d_grad_out.
 */
#define UWIE_LOSS_IDENTITY 0
#define UWIE_LOSS_VGG 1
#define UWIE_LOSS_GATED 2
size_t uwie_ref_loss_workspace_bytes(int batch, int H, int W);
int uwie_ref_loss_f32(uwie_ctx *ctx, int map, const float *d_img, const float *d_params, int flags, int planar, int batch, int H,
                      int W, const float *d_ref, float *d_out, float *d_saved, float *d_loss, void *d_workspace,
                      size_t workspace_bytes, void *stream);
int uwie_ref_loss_bwd_f32(uwie_ctx *ctx, int map, const float *d_img, const float *d_params, int flags, int planar, int batch,
                          int H, int W, const float *d_saved, const float *d_ref, const float *d_grad_out,
                          const float *d_grad_loss, float *d_grad_img, float *d_grad_params, void *d_workspace,
                          size_t workspace_bytes, void *stream);
/*
 * uwie_device_status without the wait: enqueues on `stream` a copy of the status word to d_bits (device memory, one uint32)
 * and clears the word, so that a caller can bring it back together with its own results in one copy.
 */
int uwie_device_status_async(uwie_ctx *ctx, uint32_t *d_bits, void *stream);

/*
 * PerceptualLoss (vgg_16_UIE.py:257-269; the contract: DESIGN.md section 14): d_loss [1] float32 =
 * mse_loss(F(pred), F(target)) with F = torchvision vgg16().features[:16] (conv1_1 ... relu3_3).  d_pred, d_target:
 * float32 (batch, 3, H, W), H and W >= 4 (both max-pools non-empty).  precision:
 *   UWIE_VGG_F32  float32 throughout (torch's float32 module, free summation order inside each convolution)
 *   UWIE_VGG_F16  torch.autocast's float16 contract: inputs, weights and biases rounded to float16, each convolution
 *                 accumulates in float32 and rounds its output (after the bias) to float16, ReLU and max-pool on float16,
 *                 the loss in float32; the backward rounds dL/dF and every data-gradient to float16 and returns float32.
 * The loss sums float32 terms in float64 in a fixed order (no atomics) and rounds once: the same inputs give the same bits.
 * uwie_vgg_create packs torchvision's 14 tensors, float32 on the device, flat in features.N order (weight then bias of
 * convs 0, 2, 5, 7, 10, 12, 14; UWIE_VGG_PARAMS floats in all) into a handle of one precision; d_params is not kept.
 * uwie_perceptual_f32 keeps what the backward needs in the workspace (uwie_perceptual_workspace_bytes): the workspace must
 * stay untouched until the last uwie_perceptual_bwd_f32 of that forward, which gives d_grad_pred (float32, d_pred's shape)
 * = g * dloss/dpred with g = d_grad_loss[0] read on the device (no host sync).  target gets no gradient.
 */
#define UWIE_VGG_F32 0
#define UWIE_VGG_F16 1
#define UWIE_VGG_PARAMS 1735488
typedef struct uwie_vgg uwie_vgg;
int uwie_vgg_create(uwie_ctx *ctx, const float *d_params, int precision, uwie_vgg **out_vgg);
void uwie_vgg_destroy(uwie_vgg *vgg);
size_t uwie_perceptual_workspace_bytes(int batch, int H, int W, int precision);
int uwie_perceptual_f32(uwie_ctx *ctx, const uwie_vgg *vgg, const float *d_pred, const float *d_target, int batch, int H, int W,
                        float *d_loss, void *d_workspace, size_t workspace_bytes, void *stream);
int uwie_perceptual_bwd_f32(uwie_ctx *ctx, const uwie_vgg *vgg, int batch, int H, int W, const float *d_grad_loss, float *d_grad_pred,
                            void *d_workspace, size_t workspace_bytes, void *stream);

/*
 * ImprovedVGGParameterNet.forward in eval mode (vgg_16_UIE.py:135-255; the contract: DESIGN.md section 15), float32, no
 * autograd: vgg16().features[:23] (conv1_1 ... relu3_3, pool3, conv4_1 ... relu4_3) -> the global average of relu4_3
 * per (image, channel), written twice (avgpool and the reference's "maxpool", also an AdaptiveAvgPool2d) -> [the 79
 * features] -> feature_fusion (Linear, BatchNorm1d with running statistics, ReLU; twice) -> attention product ->
 * four heads -> sigmoid(raw) * (max - min) + min.  hidden_dim is 256.
 * d_params: the state dict's float tensors, float32 on the device, flat in state-dict order without num_batches_tracked:
 *   vgg_features.N.weight, .bias for N = 0, 2, 5, 7, 10, 12, 14, 17, 19, 21;
 *   feature_fusion.0.weight [512][Din], .0.bias, .1.weight, .1.bias, .1.running_mean, .1.running_var,
 *   feature_fusion.4.weight [256][512], .4.bias, .5.weight, .5.bias, .5.running_mean, .5.running_var;
 *   attention.0.weight [64][256], .0.bias, attention.2.weight [256][64], .2.bias;
 *   param_heads.K.0.weight [128][256], .0.bias, .3.weight [1][128], .3.bias for K = omega, gamma, L_low, L_high;
 * Din = 1103 with use_features, 1024 without; UWIE_PARAM_NET_PARAMS(use_features) floats in all.  d_params is not kept.
 * uwie_param_net_f32: d_img float32 (batch, 3, H, W), H and W >= 8 (pool3 non-empty); d_features [batch][79] (required
 * for a use_features net, not read otherwise); d_out [batch][4] = omega, gamma, L_low, L_high; d_pooled (NULL: not
 * written) [batch][1024], the pooled vector.  Deterministic: the same inputs give the same bits.
 */
#define UWIE_PARAM_NET_PARAMS(use_features) ((use_features) ? 8500100 : 8459652)
typedef struct uwie_param_net uwie_param_net;
int uwie_param_net_create(uwie_ctx *ctx, const float *d_params, int use_features, uwie_param_net **out_net);
void uwie_param_net_destroy(uwie_param_net *net);
size_t uwie_param_net_workspace_bytes(int batch, int H, int W);
int uwie_param_net_f32(uwie_ctx *ctx, const uwie_param_net *net, const float *d_img, const float *d_features, int batch, int H, int W,
                       float *d_out, float *d_pooled, void *d_workspace, size_t workspace_bytes, void *stream);

/*
 * deep_learning_parameters.ParameterPredictor.forward in eval mode (deep_learning_parameters.py:97-163; DESIGN.md section
 * 17), float32, no autograd: Linear(feature_dim, hidden) + ReLU -> num_blocks residual blocks relu(W2 relu(W1 x + b1) + b2 + x)
 * -> Linear(hidden, hidden / 2) + ReLU -> four heads Linear(hidden / 2, 1) + sigmoid with the ranges of :158-161 (Dropout is
 * the identity).  d_params: the state dict's tensors, float32 on the device, flat in state_dict() order:
 *   input_proj.0.weight [hidden][feature_dim], .bias; res_blocks.N.block.0.weight [hidden][hidden], .bias, .block.3.weight,
 *   .bias for N = 0 .. num_blocks - 1; output_proj.0.weight [hidden / 2][hidden], .bias; param_heads.K.weight [1][hidden / 2],
 *   .bias for K = gamma, L_low, L_high, use_gamma.  d_params is not kept.
 * hidden_dim even, 2 .. 1152; feature_dim 1 .. 1152; num_blocks 0 .. 64 (UWIE_E_INVALID otherwise).
 * uwie_mlp_forward: d_features [batch][feature_dim], float64 (features_are_f64, what uwie_feature_extractor_u8 writes; each
 * value is rounded to float32 as it is loaded, torch's .float()) or float32; d_out [batch][4] float32 = L_low, L_high,
 * use_gamma, gamma: the gated module's d_params.  batch 1 .. 2^20.  Deterministic: one wave per neuron sums in a fixed order,
 * so a row's result does not depend on the batch it is in.  Workspace: uwie_mlp_workspace_bytes(batch, hidden_dim) (0: out
 * of range).
 */
typedef struct uwie_mlp uwie_mlp;
int uwie_mlp_create(uwie_ctx *ctx, const float *d_params, int feature_dim, int hidden_dim, int num_blocks, uwie_mlp **out_net);
void uwie_mlp_destroy(uwie_mlp *net);
size_t uwie_mlp_workspace_bytes(int batch, int hidden_dim);
int uwie_mlp_forward(uwie_ctx *ctx, const uwie_mlp *net, const void *d_features, int features_are_f64, int batch, float *d_out,
                     void *d_workspace, size_t workspace_bytes, void *stream);

/*
 * EndToEndTrainer.train_epoch's step for ParameterPredictor (deep_learning_parameters.py:265-306):
 * the train-mode forward (:149-163 with the Dropouts of :104, :108, :127 live), its backward (loss.backward(), :288), and
 * clip_grad_norm_ with torch.optim.Adam (:262, :291-293).  A trainer owns the parameters, the gradients and Adam's two
 * moments, float32 on the device.  d_params / d_buf: flat in state_dict() order, all tensors, as uwie_mlp_create takes it.
 * uwie_mlp_trainer_create: the limits of uwie_mlp_create; the moments and the step count start at 0.
 * uwie_mlp_train_forward: d_features, d_out as uwie_mlp_forward; batch 1 .. 65536.  p in [0, 1): every Dropout's rate; a
 *   dropped value is x * 0, a kept one x * float32(1 / (1 - p)); p = 0 has no dropout and gives uwie_mlp_forward's bits.
 *   There are 1 + 2 * num_blocks sites of [batch][hidden], in call order: input_proj.2, then per block block.2 and dropout.
 *   mask_mode UWIE_MASKS_GIVEN: d_masks uint8 [sites][batch][hidden], nonzero keeps (required when p > 0).
 *   UWIE_MASKS_DRAWN: the keep bit of (site, row, column) is drawn by Philox4x32-10 from (seed, the trainer's step count, site,
 *   row, column) alone; d_masks (NULL: not written) receives the masks.  The workspace
 *   (uwie_mlp_train_workspace_bytes, 0: out of range) keeps what the backward needs and must stay untouched until it ran.
 * uwie_mlp_backward: the gradients of the last uwie_mlp_train_forward (same d_features, batch, workspace) given d_grad_out
 *   [batch][4] in the gated order, as uwie_ref_loss_bwd_f32 writes d_grad_params; its first two columns are never read.
 *   Overwrites the trainer's gradients (zero_grad); the L_low and L_high heads get exact zeros.  Deterministic.
 * uwie_mlp_adam_step: total_norm over all tensors but the L_low / L_high heads (they have no gradient in the reference, so
 *   torch skips them), gradients *= min(max_norm / (total_norm + 1e-6), 1), then Adam's update with the step count + 1
 *   (no weight decay); those heads stay as they are.  d_norm (NULL: not written): one float64, total_norm.  No host read.
 * uwie_mlp_trainer_get / _set: copy one of the four arrays to / from d_buf; they wait for the device.
 * uwie_mlp_trainer_eval: uwie_mlp_forward on the current weights (workspace: uwie_mlp_workspace_bytes).
 */
#define UWIE_MASKS_GIVEN 0
#define UWIE_MASKS_DRAWN 1
#define UWIE_TRAINER_PARAMS 0
#define UWIE_TRAINER_GRADS 1
#define UWIE_TRAINER_EXP_AVG 2
#define UWIE_TRAINER_EXP_AVG_SQ 3
typedef struct uwie_mlp_trainer uwie_mlp_trainer;
int uwie_mlp_trainer_create(uwie_ctx *ctx, const float *d_params, int feature_dim, int hidden_dim, int num_blocks,
                            uwie_mlp_trainer **out_trainer);
void uwie_mlp_trainer_destroy(uwie_mlp_trainer *trainer);
size_t uwie_mlp_train_workspace_bytes(int batch, int hidden_dim, int num_blocks);
int uwie_mlp_train_forward(uwie_ctx *ctx, uwie_mlp_trainer *trainer, const void *d_features, int features_are_f64, int batch, double p,
                           int mask_mode, uint8_t *d_masks, uint64_t seed, float *d_out, void *d_workspace, size_t workspace_bytes,
                           void *stream);
int uwie_mlp_backward(uwie_ctx *ctx, uwie_mlp_trainer *trainer, const void *d_features, int features_are_f64, int batch,
                      const float *d_grad_out, void *d_workspace, size_t workspace_bytes, void *stream);
int uwie_mlp_adam_step(uwie_ctx *ctx, uwie_mlp_trainer *trainer, double lr, double beta1, double beta2, double eps, double max_norm,
                       double *d_norm, void *stream);
int uwie_mlp_trainer_get(uwie_mlp_trainer *trainer, int which, float *d_buf);
int uwie_mlp_trainer_set(uwie_mlp_trainer *trainer, int which, const float *d_buf);
long long uwie_mlp_trainer_step_count(const uwie_mlp_trainer *trainer);
int uwie_mlp_trainer_set_step_count(uwie_mlp_trainer *trainer, long long step);
int uwie_mlp_trainer_eval(uwie_ctx *ctx, const uwie_mlp_trainer *trainer, const void *d_features, int features_are_f64, int batch,
                          float *d_out, void *d_workspace, size_t workspace_bytes, void *stream);

/*
 * u8.astype(float32) / 255.0 of n bytes in any layout (each value (float)v / 255.0f, IEEE division): the float image of
 * EnhancementPredictor.enhance_image (use_trained_model.py:48-51) for decoded frames, kept in their [H][W][3] layout.
 * d_in 4-byte aligned, d_out 16-byte aligned; no workspace.
 */
int uwie_u8_to_f32(uwie_ctx *ctx, const uint8_t *d_in, float *d_out, size_t n, void *stream);

/*
 * vgg_16_UIE.extract_all_features (vgg_16_UIE.py:435-466) for uint8 frames: d_features [batch][79] float32 =
 * {mean, std, min, max, median} of each channel of img = u8/255, then mean(img), std(img), mean(img**2), zeros.
 * NumPy float32 arithmetic (pairwise sums over 8192-element buffers) reproduced bit for bit.
 */
int uwie_extract_features_u8(uwie_ctx *ctx, const uint8_t *d_in, float *d_features, int batch, int H, int W,
                             void *d_workspace, size_t workspace_bytes, void *stream);

/*
 * cv2.resize(frame, (out_w, out_h)) (default INTER_LINEAR) of a batch of decoded RGB u8 frames, the per-frame preparation of
 * deep_learning_parameters.EnhancementDataset (:214-247), vgg_16_UIE.ImprovedEnhancementDataset (:335-422) and
 * use_trained_model.EnhancementPredictor._preprocess_for_vgg (:39-46).  OpenCV's fixed-point u8 path: a copy when the size
 * does not change, INTER_AREA's fast path for an exact 2x reduction, otherwise two taps per axis with 11-bit coefficients
 * and VResizeLinearVec_32s8u's rounding (DESIGN.md section 11 states the contract and its unpinned parts).
 * d_desc: DEVICE table of `batch` descriptors, one per frame: a device pointer to a contiguous [H][W][3] frame (row stride
 * 3 * W) and its size; frames may differ in size.  A descriptor outside the limits below sets UWIE_STATUS_RESIZE_DESC.
 * d_flips (optional): [batch] u8, bit UWIE_FLIP_LR = np.fliplr and bit UWIE_FLIP_UD = np.flipud of the resized frame.
 * Outputs, each optional (NULL = not written, at least one):
 *   d_out_u8   [batch][out_h][out_w][3] the resized frames;
 *   d_out_f32  [batch][3][out_h][out_w] float32 (float)v / 255.0f (IEEE division, as NumPy's astype(float32) / 255.0);
 *   d_out_norm [batch][3][out_h][out_w] float32 ((float)v / 255.0f - mean3[c]) / std3[c], each operation rounded once
 *              (torchvision's Normalize on float32 tensors); mean3 / std3 are host arrays of 3, required with d_out_norm.
 * Every output element depends on its own frame only: the bytes do not depend on the batch or on the launch shape.
 * UWIE_E_INVALID: batch, out_h or out_w < 1, batch > 65535, out_h or out_w > UWIE_RESIZE_MAX_SIDE, every output NULL.
 */
#define UWIE_RESIZE_MAX_SIDE 4096
#define UWIE_RESIZE_MAX_SRC 32768
#define UWIE_FLIP_LR 1
#define UWIE_FLIP_UD 2
typedef struct uwie_frame_desc {
    const uint8_t *data; /* device pointer to [H][W][3] u8 */
    int32_t H, W;
} uwie_frame_desc;
int uwie_resize_rgb_u8(uwie_ctx *ctx, const uwie_frame_desc *d_desc, int batch, int out_h, int out_w, const uint8_t *d_flips,
                       uint8_t *d_out_u8, float *d_out_f32, float *d_out_norm, const float *mean3, const float *std3,
                       void *stream);

/*
 * QualityAssessment.comprehensive_assessment (quality_assessment.py:215-286; called on every strategy output by
 * main.py:130-146 to pick the best one).  d_u8: the quantised frame (img*255).astype(uint8), [batch][H][W][3];
 * d_f32 (optional): the float image itself, used by the colourfulness score only (NULL: u8/255 is used).
 * weights8 (host pointer, optional): weights in the order contrast, sharpness, entropy, saturation, brightness,
 * edge_density, colorfulness, naturalness (NULL: the reference defaults).  d_scores: [batch][9] float64 = the eight
 * scores in that order, then the weighted total.  Integer-derived parts are exact; float statistics are evaluated in
 * float64 (NumPy: float32 pairwise): 2e-3 on the 0..100 scores against the float32 reference, whose own distance from a
 * float64 evaluation is at most 4.2e-5 per score on frames up to 1080p.  Against that float64 evaluation
 * (tests/quality_ref.py): 1e-9 for every score when d_f32 is NULL (functions of integer sums and histograms only); with
 * d_f32 the colourfulness reads float32 values and is held to 7e-6.  A NaN in d_f32 gives NaN colourfulness and a NaN total.
 * Deterministic: a frame's nine numbers are the same bits in every run and at every position of every batch (integer
 * atomics, and per-block float64 partials added in block order; the grid depends on H * W only).
 * Workspace: uwie_workspace_bytes(batch, H, W, NULL) (it includes the partials' [batch][blocks][4] float64 slab).
 */
int uwie_quality_scores(uwie_ctx *ctx, const uint8_t *d_u8, const float *d_f32, int batch, int H, int W, int gray_shift,
                        const double *weights8, double *d_scores, void *d_workspace, size_t workspace_bytes, void *stream);

/*
 * feature_extraction.FeatureExtractor.extract_all_features (feature_extraction.py:252-295; main.py:116 builds the classifier's
 * training rows with it, main.py:420 predicts with it).  d_u8: the quantised frames (img * 255).astype(uint8), [batch][H][W][3];
 * d_f32 (optional): the float image itself, [batch][H][W][3] float32, read by the RGB block only (feature_extraction.py:69-76;
 * NULL: u8 / 255).  d_features: [batch][uwie_feature_extractor_count(H, W)] float64 in the reference's order:
 *   0-34  extract_color_features (:17-79): LAB L, a, b mean / std / skew / kurtosis (SciPy's NaN when m2 <= (eps32 * mean)^2),
 *         HSV mean / std, colour cast factor, M, D, mean a, mean b, then R, G, B mean / std / min / max
 *   35-56 extract_texture_features (:81-126): uniform LBP (P = 8, R = 1) histogram, GLCM props of the 128x128 resize
 *   57-61 extract_frequency_features (:128-165): DCT energy fractions, mean and std of |dct|; absent when H or W is odd and
 *         greater than 1 (cv2.dct refuses; the reference's try / except drops the block): 74 values then
 *   ...   extract_edge_features (:167-206): Sobel, Canny (50, 150) density, Laplacian (ksize 3); extract_quality_features
 *         (:208-250): contrast, entropy, mean, median, p25, p75, range, saturation mean / std, RMS contrast.
 * gray_shift: RGB2GRAY coefficients (15: OpenCV 4.x; 14: older).  Histogram- and integer-derived values are exact; the float
 * statistics are evaluated in float64 (NumPy: float32); the DCT is float32 MFMA.  Results do not depend on the batch.
 * A frame's histograms that do not count every pixel set UWIE_STATUS_FEATURE_COUNTS.
 * Workspace: uwie_workspace_bytes_feature_extractor(batch, H, W) (about 6 bytes per pixel with the DCT, 1 without).
 */
int uwie_feature_extractor_count(int H, int W);
size_t uwie_workspace_bytes_feature_extractor(int batch, int H, int W);
int uwie_feature_extractor_u8(uwie_ctx *ctx, const uint8_t *d_u8, const float *d_f32, int batch, int H, int W, int gray_shift,
                              double *d_features, void *d_workspace, size_t workspace_bytes, void *stream);

/*
 * The labelling loop of main.py:118-146 for a batch: every parameter set ps[0 .. n-1] (Config.STRATEGIES, config.py:28-75:
 * five DICT sets; SIX sets are accepted too) is applied to the frames, QualityAssessment.comprehensive_assessment
 * (quality_assessment.py:215-286) scores each result, and the best one per frame -- the FIRST maximum of the weighted total in
 * the sets' order, like max(strategy_scores, key=strategy_scores.get) (main.py:145) -- is selected, all on the device.
 * Consecutive DICT dehazing sets share one atmospheric-light quadtree (ES:353,379,425 evaluate the same function of the frame).
 *   d_scores [n][batch][9] float64: eight scores + weighted total per (set, frame); weights8 as in uwie_quality_scores;
 *   d_best   [batch] int32: index of the winning set;  d_best_u8 (optional) [batch][H][W][3]: its (y * 255).astype(uint8);
 *   d_all_u8 (optional) [n][batch][H][W][3]: every set's output (NULL: kept in the workspace only).
 * Workspace: uwie_workspace_bytes_select(batch, H, W, ps, n, d_all_u8 != NULL).
 */
size_t uwie_workspace_bytes_select(int batch, int H, int W, const uwie_params *ps, int n, int with_outputs);
int uwie_select_best_u8(uwie_ctx *ctx, const uint8_t *d_in, int batch, int H, int W, const uwie_params *ps, int n,
                        const double *weights8, uint8_t *d_best_u8, int32_t *d_best, double *d_scores, uint8_t *d_all_u8,
                        void *d_workspace, size_t workspace_bytes, void *stream);

/*
 * UCIQE and UIQM, the two no-reference metrics the underwater-enhancement literature reports, in a fixed form.  An extension
 * without a reference counterpart (like uwie_params.dark_patch): this comment is the contract, tests/uw_quality_ref.py restates
 * it in NumPy.  The papers' PLIP operators and image-dependent block counts are left out on purpose: 8 x 8 blocks, plain
 * arithmetic, so that almost everything is a function of integer histograms and integer block extrema.
 *
 * Input: a u8 RGB frame, H x W, n = H * W pixels.  All arithmetic not marked integer is float64.
 *   UCIQE  (L8, a8, b8) = the 8-bit LAB triple of uwie_rgb2lab_u8; da = a8 - 128, db = b8 - 128; C = sqrt(da^2 + db^2) / 255.
 *          sigma_c = population standard deviation of C over the frame.
 *          con_l   = (L8 sorted ascending at index min(99 * n / 100, n - 1)  -  L8 sorted ascending at index n / 100) / 255
 *                    (integer divisions).
 *          mu_s    = mean over all n pixels of sqrt(da^2 + db^2) / L8 where L8 > 0, and of 0 where L8 = 0.
 *          UCIQE   = 0.4680 * sigma_c + 0.2745 * con_l + 0.2576 * mu_s.
 *   UIQM   = 0.0282 * UICM + 0.2953 * UISM + 3.5753 * UIConM.  The 8 x 8 blocks below are the (H / 8) x (W / 8) full blocks counted
 *          from the top left corner; remainder rows and columns are ignored; with no block (H < 8 or W < 8) UISM = UIConM = 0.
 *          UICM    RG = R - G (integer, -255 .. 255) and YB2 = R + G - 2 B (integer, -510 .. 510).  Of each plane, sorted
 *                  ascending, the t = n / 10 smallest and the t largest values are dropped; m = n - 2 t >= 1 remain; mu = their mean,
 *                  var = the mean of (x - mu)^2 over them.  mu_YB = mu_YB2 / 2, var_YB = var_YB2 / 4.
 *                  UICM = -0.0268 * sqrt(mu_RG^2 + mu_YB^2) + 0.1586 * sqrt(var_RG + var_YB).
 *          UISM    per channel c: gx, gy = the 3 x 3 Sobel responses (-1 0 1 / -2 0 2 / -1 0 1 and its transpose) of the channel's
 *                  bytes, BORDER_REFLECT_101 at the frame's border; q = min(gx^2 + gy^2, 65025) * c^2 with c the pixel's byte
 *                  (an integer <= 65025^2 < 2^32).  A block's term is ln(q_max / q_min) over its 64 pixels if q_min > 0, else 0;
 *                  EME_c = the mean of the terms over the blocks; UISM = 0.299 * EME_R + 0.587 * EME_G + 0.114 * EME_B.
 *                  (The EME of the map edge magnitude x channel; the ratio of two products is taken on their exact squares.)
 *          UIConM  g = the gray byte (uwie_rgb2gray_u8 with gray_shift); per block M, m = its extrema, r = (M - m) / (M + m);
 *                  the block's term is r * ln r if M > m, else 0; UIConM = minus the mean of the terms.
 * A frame of one gray level scores 0 in all eight; the sign of a zero is not part of the contract.
 *
 * d_scores: [batch][UWIE_UW_SCORES] float64 = sigma_c, con_l, mu_s, UCIQE, UICM, UISM, UIConM, UIQM.
 * Exact: con_l, UICM's moments (integer sums from the 256-, 511- and 1021-bin histograms up to the last divisions), every block's
 * extrema and branch.  sigma_c and mu_s are float64 sums over the pixels; against the float64 evaluation every score is held
 * to 1e-9 (tests/test_gpu_uw_quality.py).  Deterministic as uwie_quality_scores: a frame's eight numbers are the same bits in
 * every run and at every position of every batch (integer atomics, float64 partials per block and per tile added in their
 * order; the grids depend on H and W only).  A fixed number of launches, no host read.  batch <= 65535.
 * uwie_underwater_plan: the tile (*tile_w x *tile_h pixels, multiples of 8, anchored at the frame's top left corner) that one
 * workgroup of the block pass stages with a one-pixel halo: the launcher runs on these numbers, so a test can aim at the seams.
 * Workspace: uwie_workspace_bytes_underwater(batch, H, W) (7 KB per frame plus at most 48 bytes per 1024 pixels).
 */
#define UWIE_UW_SCORES 8
size_t uwie_workspace_bytes_underwater(int batch, int H, int W);
int uwie_underwater_plan(int H, int W, int *tile_w, int *tile_h);
int uwie_underwater_scores_u8(uwie_ctx *ctx, const uint8_t *d_u8, int batch, int H, int W, int gray_shift, double *d_scores,
                              void *d_workspace, size_t workspace_bytes, void *stream);

/*
 * best[b] = the FIRST maximum over the n sets, in their order, of d_scores[k][b][col] (d_scores: [n][batch][ncols] float64; the
 * pick of uwie_select_best_u8 generalised over the column).  With d_all_u8 [n][batch][H][W][3] and d_best_u8 [batch][H][W][3]
 * (both optional, given together) the winner's frame is gathered: d_best_u8[b] = d_all_u8[best[b]][b].  Without them H and W
 * are not read.  n: 1 .. 65535; a NaN never beats the running maximum.
 */
int uwie_pick_best_u8(uwie_ctx *ctx, const double *d_scores, int n, int batch, int ncols, int col, const uint8_t *d_all_u8, int H,
                      int W, int32_t *d_best, uint8_t *d_best_u8, void *stream);

/*
 * Full-reference quality of a result against its ground truth: mean absolute error, mean squared error, PSNR and SSIM (Wang et
 * al. 2004; the definition of MATLAB's ssim.m and of scikit-image's structural_similarity(gaussian_weights=True,
 * use_sample_covariance=False, data_range=255)).  An extension without a reference counterpart: this comment is the contract,
 * tests/ref_quality_ref.py restates it in NumPy.
 *
 * Input: two u8 RGB frames of the same H x W, the result x and the reference y; n = H * W.  All arithmetic not marked integer
 * is float64.
 *   mae   = (integer sum of |x - y| over all 3 n bytes) / (3 n).
 *   mse   = (integer sum of (x - y)^2 over all 3 n bytes) / (3 n).  Both sums are exact integers below 2^53: each column is one
 *           correctly rounded division.
 *   psnr  = 10 * log10(65025 / mse); +inf where mse = 0.
 *   SSIM of a plane pair (px, py) of bytes:
 *           window   11 x 11 Gaussian, sigma = 1.5, separable: the 1-D taps are w[k] = exp(-(k - 5)^2 / 4.5), k = 0 .. 10, divided
 *                    by their float64 sum taken in index order.
 *           C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2.
 *           Windows lie wholly inside the frame ("valid"): the map has (H - 10) x (W - 10) points, point (i, j) covering rows
 *           i .. i + 10 and columns j .. j + 10.  No border rule exists.
 *           Five window sums per point, of x, y, x * x, y * y and x * y (the products are exact integers).  Order of summation:
 *           along the row first, the 11 taps added in index order (r[j] = w[0] v[j] + w[1] v[j + 1] + ... from the left), then
 *           down the column in index order.  (The device adds down the column in this order; along the row it first adds the
 *           two values that share a tap, w[k] = w[10 - k], as exact integers; it uses fused multiply-adds.  See the tolerance.)
 *           mu_x = sum w x, mu_y = sum w y; population form: var_x = sum w x^2 - mu_x^2, var_y likewise, cov = sum w x y - mu_x mu_y.
 *           s = (2 mu_x mu_y + C1) (2 cov + C2) / ((mu_x^2 + mu_y^2 + C1) (var_x + var_y + C2)).
 *           The plane's SSIM is the mean of s over the map.
 *   ssim_y          SSIM of the gray bytes (uwie_rgb2gray_u8 with gray_shift) of the two frames.
 *   ssim_r, _g, _b  SSIM of the channel bytes.
 *   ssim_rgb        (ssim_r + ssim_g + ssim_b) / 3, added in that order.
 *   With H < 11 or W < 11 there is no window and the five SSIM columns are NaN (uwie_pick_best_u8 never lets a NaN win).
 * Two identical frames score mae = mse = 0, psnr = +inf and every SSIM exactly 1.0: the x and the y side are computed by the
 * same operations in the same order, so numerator and denominator of every s are the same bits.  Part of the contract.
 *
 * d_scores: [batch][UWIE_REF_SCORES] float64 = mae, mse, psnr, ssim_y, ssim_r, ssim_g, ssim_b, ssim_rgb.
 * Frame i of d_u8 [batch][H][W][3] is compared with frame i % ref_batch of d_ref_u8 [ref_batch][H][W][3]; 1 <= ref_batch <= batch
 * and batch % ref_batch == 0, so the outputs of n strategies [n * B] share B references without copies.
 * Exact: mae and mse (integer sums up to the division).  psnr is held to 1e-9 relative and every SSIM column to 1e-9 absolute
 * against the float64 evaluation (tests/test_gpu_ref_quality.py): window sums of values <= 65025 carry a few 1e-11 of absolute
 * error in any order of summation, both factors of the denominator are at least C1 and C2, and a mean does not amplify.
 * Deterministic as uwie_underwater_scores_u8: integer partials per block, one float64 partial per tile and plane, added in
 * their order; the grids depend on H and W only, so a frame's eight numbers are the same bits in every run and at every
 * position of every batch.  Three launches (two without a window), no memset, no host read.  batch <= 65535.
 * uwie_reference_plan: the tile of map points (*tile_w x *tile_h, anchored at the map's top left corner) that one workgroup of
 * the SSIM pass produces from a (*tile_h + 10) x (*tile_w + 10) patch of both frames; the launcher runs on these numbers, so a
 * test can aim at the seams.  Workspace: uwie_workspace_bytes_reference(batch, H, W) (at most 4 KB per frame plus 32 bytes per tile).
 */
#define UWIE_REF_SCORES 8
size_t uwie_workspace_bytes_reference(int batch, int H, int W);
int uwie_reference_plan(int H, int W, int *tile_w, int *tile_h);
int uwie_reference_scores_u8(uwie_ctx *ctx, const uint8_t *d_u8, const uint8_t *d_ref_u8, int batch, int ref_batch, int H, int W,
                             int gray_shift, double *d_scores, void *d_workspace, size_t workspace_bytes, void *stream);

/*
 * Gray-world white balance with red-channel compensation, the pre-pass of the underwater literature: Ancuti et al. 2018, "Color
 * Balance and Fusion for Underwater Image Enhancement", eq. 4-5, followed by gray-world (Buchsbaum), in byte units.  An
 * extension without a reference counterpart (the reference's white_balance is a percentile stretch, its cast handling a fixed
 * x 0.85; both stay what they are): this comment is the contract, tests/gray_world_ref.py restates it in NumPy.
 *
 * Input: a u8 RGB frame, H x W, n = H * W pixels with bytes (r, g, b).  Parameters red, blue, max_gain: 0 <= red, blue <= 1 (the
 * papers' alpha), max_gain = 0 (no bound) or >= 1.  Anything marked integer is exact integer arithmetic.  Everything else is
 * float64, each operation rounded once, no fused multiply-add.  Integers are converted exactly; all of them are below 2^53.
 *
 *   S_r = sum r   S_g = sum g   S_b = sum b   S_rg = sum r * g   S_bg = sum b * g          (integer, over the n pixels)
 *   N = n         mean_r = S_r / N   mean_g = S_g / N   mean_b = S_b / N
 *   k_r = (red  * max(mean_g - mean_r, 0)) / 65025        k_b = (blue * max(mean_g - mean_b, 0)) / 65025
 *      compensated value of a pixel, real-valued:  r' = r + k_r * (255 - r) * g,  g' = g,  b' = b + k_b * (255 - b) * g
 *      (I_rc = I_r + alpha (mean(I_g) - mean(I_r)) (1 - I_r) I_g with I = byte / 255; compensation never darkens: the max)
 *   m_r = (S_r + k_r * (255 * S_g - S_rg)) / N      m_g = mean_g      m_b = (S_b + k_b * (255 * S_g - S_bg)) / N
 *      (255 * S_g - S_rg is one exact integer; m_c is the mean of the compensated channel, in closed form)
 *   gray = ((m_r + m_g) + m_b) / 3
 *   s_c  = gray / m_c  if m_c > 0,  else 1 ;   if max_gain > 0:  s_c = min(s_c, max_gain)
 *   c_r  = s_r * k_r        c_b = s_b * k_b
 *   w_r  = s_r * r + c_r * ((255 - r) * g)          (integer product, two multiplications, one addition)
 *   w_g  = s_g * g
 *   w_b  = s_b * b + c_b * ((255 - b) * g)
 *   out_c = rint(min(w_c, 255))                     (round half to even; w_c >= 0 always, NaN cannot arise)
 *
 * Fixed by this: a frame of one gray level, and a black frame, come back unchanged with gains exactly 1; with red = blue = 0 the
 * stage is plain gray-world; with alpha <= 1 a compensated value never exceeds 255 before the gain.
 *
 * d_stats: [batch][UWIE_GW_STATS] float64 = mean_r, mean_g, mean_b, k_r, k_b, m_r, m_g, m_b, gray, s_r, s_g, s_b.  Each frame of a
 * batch has its own sums and gains.  d_out [batch][H][W][3] and d_stats are each optional, not both NULL; with d_out == NULL
 * only the sum pass and the coefficients run.  d_out == d_in (exactly; a partial overlap is an error) is allowed.  d_in and d_out
 * are 4-byte aligned, d_stats 8-byte; a frame inside a batch starts wherever 3 * H * W puts it.  batch <= 65535.
 * Out-of-range or non-finite parameters are UWIE_E_INVALID with a message naming the field, a short or NULL workspace
 * UWIE_E_WORKSPACE; every check runs before the context is touched.
 * Exact: every byte and every stat equals the float64 evaluation above bit for bit (tests/test_gpu_gray_world.py): the sums are
 * integers, so no order of summation enters.  At most three launches (two without d_out), no atomics, no memset, no host read;
 * the grids depend on H and W only, so a frame's results are the same bits in every run and at every position of every batch.
 * uwie_gray_world_plan: *block_px = the pixels one workgroup of the sum pass adds into 32-bit integers (65025 * *block_px < 2^32),
 * *thread_px = the pixels one thread of the apply pass takes per step; a frame's last n % *thread_px pixels go byte by byte.  The
 * launchers run on these numbers, so a test can aim at the seams.
 * Workspace: uwie_workspace_bytes_gray_world(batch, H, W) (per frame 32 bytes per started *block_px pixels and 96 bytes of stats, each of the two
 * arrays rounded up to 256 bytes).
 */
#define UWIE_GW_STATS 12
size_t uwie_workspace_bytes_gray_world(int batch, int H, int W);
int uwie_gray_world_plan(int H, int W, int *block_px, int *thread_px);
int uwie_gray_world_u8(uwie_ctx *ctx, const uint8_t *d_in, int batch, int H, int W, double red, double blue, double max_gain,
                       uint8_t *d_out, double *d_stats, void *d_workspace, size_t workspace_bytes, void *stream);

/*
 * Multi-scale fusion, the second half of Ancuti et al. 2018, "Color Balance and Fusion for Underwater Image Enhancement" (the
 * gray-world pre-pass above is its first): from the balanced frame a gamma-corrected and a sharpened input are derived, each
 * gets a weight from Laplacian contrast, saliency and saturation, and the two are blended over a Laplacian pyramid.  An
 * extension without a reference counterpart: this comment is the contract, tests/fusion_ref.py restates it in NumPy.
 *
 * Input: a u8 RGB frame x, H x W, n = H * W pixels; the caller has balanced it already.  Parameters: gamma, finite,
 * 0 < gamma <= 8; levels L, 1 <= L <= 8; gray_shift, 14 or 15.  "Integer" is exact integer arithmetic.  Everything else is
 * float64, each operation rounded once, in the order written, no fused multiply-add; integers are converted exactly.  Every
 * out-of-range index is clamped to the plane (BORDER_REPLICATE), so every size from 1 x 1 is valid at every L.
 *
 * The 5-tap rule along an axis:  T(v)[j] = ((v[j-2] + v[j+2]) + 4 * (v[j-1] + v[j+1])) + 6 * v[j].
 *   B(p) = T along the row, then T down the column (the taps of the 5 x 5 binomial, summing to 256).
 *
 * The two inputs (integer, bytes):
 *   I1_c = G[x_c],  G[v] = rint(255 * (v / 255)^gamma): a 256-entry byte table built on the host with C pow();
 *          uwie_fusion_table(gamma, table) returns it (host only, no context, no device).
 *   I2_c = clamp((512 * x_c - B(x_c) + 128) >> 8, 0, 255)     (>> is the arithmetic shift: floor)
 *          an unsharp mask of amount 1 over the binomial blur, x + (x - blur(x)).  The paper's normalising stretch is replaced
 *          by the clamp, on purpose: the input is a byte and needs no second global pass.
 *
 * The weight of input k (k = 1, 2), per pixel, with (r, g, b) the bytes of I_k:
 *   Y    = the gray byte of I_k (the rule of uwie_rgb2gray_u8 with gray_shift)
 *   lap  = |4 * Y - Y(up) - Y(down) - Y(left) - Y(right)|   (integer)          wl = lap / 255
 *   S_c  = the sum of I_k's channel c over the frame (integer)                  mu_c = S_c / n
 *   d_c  = mu_c - B(I_k,c) * 2^-8        (B is an integer, the scaling exact)
 *   sal  = ((0 + d_r * d_r) + d_g * d_g) + d_b * d_b                            ws = sal / 65025
 *          (the saliency of Achanta et al. -- distance of the blurred pixel from the frame's mean -- on the RGB bytes, not Lab)
 *   q    = (r - Y)^2 + (g - Y)^2 + (b - Y)^2                (integer)          wsat = sqrt(q / 3) / 255
 *   W_k  = (wl + ws) + wsat
 * The normalised weight of input 1:   a = W_1 + 0.1     Wn = a / (a + (W_2 + 0.1))
 *   Input 2's weight is 1 - Wn at every level: reduce() below maps a constant plane to itself exactly, so the Gaussian
 *   pyramid of 1 - Wn is one minus that of Wn.
 *
 * The pyramid.  A level has ceil(h / 2) x ceil(w / 2) points of the h x w level above it.
 *   reduce(p):  T along the row, T down the column, times 2^-8, sampled at the even indices.
 *   expand(p) to a given finer size, along the row and then down the column; with k = i / 2 (integer):
 *       even i:  ((p[k-1] + p[k+1]) + 6 * p[k]) * 0.125          odd i:  (p[k] + p[k+1]) * 0.5
 *
 * The fusion, per channel:
 *   D = I1 - I2  (integer)      GW_0 = Wn    GD_0 = D     GW_l = reduce(GW_l-1)    GD_l = reduce(GD_l-1)
 *   acc_L-1 = GW_L-1 * GD_L-1
 *   for l = L-2 .. 0:   acc_l = GW_l * (GD_l - expand(GD_l+1)) + expand(acc_l+1)
 *   out = rint(min(max(I2 + acc_0, 0), 255))                                    (round half to even)
 * Two inputs whose weights sum to one give  sum_k G_l(Wn_k) * L_l(I_k) = L_l(I2) + G_l(Wn_1) * L_l(I1 - I2), and the collapse is
 * linear: this is the paper's multi-scale fusion with one weight pyramid and one pyramid of the difference instead of two and
 * two.  That is the definition, not an optimisation behind it.
 *
 * Fixed by this: a frame of one level v comes back as rint((G[v] + v) / 2) at every L (Wn = 0.5 exactly; 77 at gamma 2.2 gives
 * 48 from 47.5); L = 1 is the per-pixel blend I2 + Wn * D.
 *
 * d_out [batch][H][W][3].  Optional outputs, NULL to skip: d_in1, d_in2 ([batch][H][W][3], the two inputs) and d_weight
 * ([batch][H][W] float64, Wn, 8-byte aligned), so that a wrong byte can be traced to a stage.  d_out == d_in is allowed; any
 * other overlap among d_in, d_out, d_in1, d_in2 is an error.  No alignment is asked of the byte planes; a frame inside a batch
 * starts wherever 3 * H * W puts it.  batch <= 65535.  Out-of-range or non-finite parameters are UWIE_E_INVALID with a message
 * naming the field, a short or NULL workspace UWIE_E_WORKSPACE; every check runs before the context is touched.
 * Exact: every byte of d_out, d_in1, d_in2 and every bit of d_weight equals the float64 evaluation above
 * (tests/test_gpu_fusion.py).  2 * L + 2 launches whatever H and W, no atomics, no memset, no host read; the grids come from H,
 * W and L only, so a frame's results are the same bits in every run and at every position of every batch.
 * uwie_fusion_plan: *tile_w x *tile_h = the level-0 tile one workgroup stages with its 2-pixel halo; the launchers run on these
 * numbers, so a test can aim at the seams.
 * Workspace: uwie_workspace_bytes_fusion(batch, H, W, levels): per pixel 3 bytes of I2, 8 of Wn and 6 of D, per point of each
 * coarser level 56 bytes (GW, GD, acc in float64), 32 bytes per level-0 tile and 64 per frame.
 */
size_t uwie_workspace_bytes_fusion(int batch, int H, int W, int levels);
int uwie_fusion_plan(int H, int W, int levels, int *tile_w, int *tile_h);
int uwie_fusion_table(double gamma, uint8_t *table256); /* host only */
int uwie_fusion_u8(uwie_ctx *ctx, const uint8_t *d_in, int batch, int H, int W, double gamma, int levels, int gray_shift,
                   uint8_t *d_out, uint8_t *d_in1, uint8_t *d_in2, double *d_weight, void *d_workspace, size_t workspace_bytes,
                   void *stream);

/* ---------------- strategy classifier: main.py:398-433 (predict) ---------------- */

/*
 * A fitted scikit-learn model of one of the three kinds train_classifier fits (main.py:271-275), with its StandardScaler,
 * as flat HOST arrays (underwater_image_enhancement_amd/classifier.py exports them).  F = n_features, C = n_classes,
 * T = n_trees, N = n_nodes, S = n_sv, P = C * (C - 1) / 2.
 *   all      mean[F], scale[F]: StandardScaler.mean_ / scale_ (zeros / ones without centring / scaling)
 *   RF, GB   tree_offset[T + 1] (root of tree t at node tree_offset[t]; tree_offset[T] = N), per node (tree-local child
 *            indices, -1 for both at a leaf): left[N], right[N], feature[N], threshold[N], missing_left[N];
 *            value: RF [N][C] (the tree_.value class fractions), GB [N] (the regression leaf value)
 *   GB       T = n_stages * K trees, stage-major, K = 1 for two classes and C otherwise; learning_rate; init[K] (the
 *            estimator's own _raw_predict_init)
 *   SVC      sv[S][F] (support_vectors_), dual_coef[C - 1][S] (_dual_coef_), intercept[P] (_intercept_: libsvm's -rho),
 *            n_support[C], prob_a[P], prob_b[P] (_probA / _probB), gamma (_gamma); RBF kernel only
 */
#define UWIE_MODEL_RF 0
#define UWIE_MODEL_GB 1
#define UWIE_MODEL_SVC 2
typedef struct uwie_model_desc {
    int32_t kind, n_features, n_classes, n_trees, n_nodes, n_sv;
    const double *mean, *scale;
    const int32_t *tree_offset, *left, *right, *feature;
    const double *threshold;
    const uint8_t *missing_left;
    const double *value;
    double learning_rate;
    const double *init;
    const double *sv, *dual_coef, *intercept;
    const int32_t *n_support;
    const double *prob_a, *prob_b;
    double gamma;
} uwie_model_desc;
typedef struct uwie_model uwie_model;

/* Host only (no context, no device).  UWIE_E_INVALID for: an unknown kind; n_features outside 1..1024; n_classes outside
 * 2..32; more than 4096 trees or 2^22 nodes; tree offsets that are not increasing from 0 to n_nodes; an internal node whose
 * feature is >= n_features or whose children are not strictly greater than itself and less than its tree's node count
 * (scikit-learn's builders always satisfy this: every walk ends within node_count steps); more than 65536 support vectors
 * or n_support not summing to n_sv; a NULL array; a non-finite mean, scale (or a zero one), threshold, value, init,
 * learning rate, gamma or coefficient. */
int uwie_model_check(const uwie_model_desc *desc);
/* uwie_model_check, then one upload of the model into a device blob of ctx's device (synchronous). */
int uwie_model_create(uwie_ctx *ctx, const uwie_model_desc *desc, uwie_model **out_model);
void uwie_model_destroy(uwie_model *model);
int uwie_model_info(const uwie_model *model, int *kind, int *n_classes, int *n_features);

/*
 * scaler.transform + classifier.predict / predict_proba (main.py:423-428) per row.  d_rows: [batch][n_features] float64,
 * unscaled; d_label: [batch] int32, the index into classes_; d_proba: [batch][n_classes] float64.  n_features must be the
 * model's.  A row's result depends on that row alone (no atomics on results, no waits between workgroups): the same bits at
 * every batch size and on every run.
 *   scaling  (x - mean) / scale in float64, each operation rounded once (StandardScaler.transform).
 *   trees    the scaled row cast to float32 (scikit-learn's DTYPE); at a node, go left iff (double)x <= threshold, or, for
 *            NaN, iff missing_left.
 *   RF       proba = ((0 + v_0) + v_1 + ...) / T over the leaves' class fractions in tree order (forest.predict_proba with
 *            n_jobs=None); label = first maximum.  Bit for bit.  NaN rows are routed (the forest accepts them).
 *   GB       raw[k] = init[k], then raw[k] += learning_rate * value[leaf] stage by stage (predict_stages): bit for bit;
 *            label = first argmax (raw >= 0 for two classes); proba = softmax (exp(raw - max) / sequential sum), or expit
 *            1 / (1 + exp(-raw)) giving [1 - p, p]: within 1e-15 (the device's exp).
 *   SVC      libsvm's svm_predict_values / svm_predict_probability: kernel exp(-gamma * |x - sv|^2) with the squared distance
 *            summed serially over features (libsvm: a BLAS ddot, order unknown), decision values within 1e-12; label = the
 *            one-vs-one vote (ties to the lower class, NOT argmax of proba); Platt sigmoid clamped to [1e-7, 1 - 1e-7] and
 *            multiclass_probability (Wu, Lin and Weng's method 2): proba within 1e-9.
 * A GB / SVC row holding NaN after scaling (scikit-learn: ValueError "Input X contains NaN") gets label -1, NaN proba, and
 * sets UWIE_STATUS_CLASSIFY_NAN.  No workspace.
 */
int uwie_classify_f64(uwie_ctx *ctx, const uwie_model *model, const double *d_rows, int batch, int n_features, int32_t *d_label,
                      double *d_proba, void *stream);
/* uwie_feature_extractor_u8 (gray_shift, d_f32 as there) followed by uwie_classify_f64 on the device, no host round trip:
 * main.py:419-428 for a batch.  d_rows (optional): [batch][79] receives the feature rows.  A frame size whose row has 74
 * values (H or W odd and > 1) against a 79-feature model is UWIE_E_INVALID before any launch.
 * Workspace: uwie_workspace_bytes_predict(batch, H, W). */
size_t uwie_workspace_bytes_predict(int batch, int H, int W);
int uwie_predict_strategy_u8(uwie_ctx *ctx, const uwie_model *model, const uint8_t *d_u8, const float *d_f32, int batch, int H,
                             int W, int gray_shift, int32_t *d_label, double *d_proba, double *d_rows, void *d_workspace,
                             size_t workspace_bytes, void *stream);

/* ---------------- per-stage entry points (parity tests, composition) ---------------- */

/* detect_image_type (S6:292-302): NumPy's sequential float32 channel means and the 3-way kind. */
int uwie_cast_classify(uwie_ctx *ctx, const uint8_t *d_in, int batch, int H, int W, int32_t *d_kind,
                       float *d_mean_rgb, void *d_workspace, size_t workspace_bytes, void *stream);

/* color_correction (S6:305-323) on x = u8/255: float32 [batch][H][W][3].  d_kind NULL = "normal". */
int uwie_normalise_correct(uwie_ctx *ctx, const uint8_t *d_in, const int32_t *d_kind, float *d_out_f32, int batch,
                           int H, int W, void *stream);

/* estimate_atmospheric_light (S6:49-113, ES:77-144): greedy quadtree descent, A = brightest pixel of
 * the leaf.  d_kind NULL = no cast correction.  d_trace (optional) receives per level, per image:
 * {y0,x0,rows,cols} as int32[4] followed by the four float64 scores, i.e. 4 int32 + 4 double = 48 bytes,
 * for at most 32 levels: [batch][32][48 bytes]. */
int uwie_atmospheric_light(uwie_ctx *ctx, const uint8_t *d_in, const int32_t *d_kind, int batch, int H, int W,
                           const uwie_params *p, float *d_A, void *d_trace, void *d_workspace,
                           size_t workspace_bytes, void *stream);

/* first half of estimate_transmission (S6:170-177 / ES:221-228): t0 = 1 - omega*min_c(x/(A+eps)) [clipped
 * on the SIX surface] as float32 [batch][H][W], and the 8-bit gray guide [batch][H][W].  p->dark_patch > 1: the dark channel
 * is eroded over the patch first (see uwie_params); the gray guide does not depend on it. */
int uwie_transmission_init(uwie_ctx *ctx, const uint8_t *d_in, const int32_t *d_kind, const float *d_A, int batch,
                           int H, int W, const uwie_params *p, float *d_t0, uint8_t *d_gray, void *stream);

/* The output tile (*tile_w x *tile_h pixels, anchored at the frame's top left corner) that one workgroup of the patched
 * transmission kernel (k_trans_patch, dark_patch = k) covers on an H x W frame: the launcher runs on these numbers, so a test
 * can aim at the seams between tiles.  No context: nothing here depends on a tuning. */
int uwie_dark_patch_plan(int H, int W, int k, int *tile_w, int *tile_h);

/* cv2.boxFilter(src, CV_64F, (k,k)) on float64 planes [batch][H][W] (S6:31-43). */
int uwie_box_filter_f64(uwie_ctx *ctx, const double *d_src, double *d_dst, int batch, int H, int W, int ksize,
                        void *d_workspace, size_t workspace_bytes, void *stream);

/* guided_filter(gray/255, t0, r, eps) followed by clip(.,0.1,1) (S6:178-180, ES:229-232): float64 [batch][H][W].
 * `exact`: 0 = fused float64 kernels (uwie_params.gf_exact = 0), 1 = cv2.boxFilter's running-sum order, 2 = fused with
 * the fixed-point a/b ring (uwie_params.inter_dtype = UWIE_INTER_FX32; the caller guarantees 0.1 <= t0 <= 1). */
int uwie_guided_filter(uwie_ctx *ctx, const uint8_t *d_gray, const float *d_t0, int batch, int H, int W, int ksize,
                       double eps, int exact, double *d_t, void *d_workspace, size_t workspace_bytes, void *stream);

/* Which rows of a frame the default float64 guided filter (gf_exact = 0, inter_dtype = F64) hands to its main kernel
 * (k_guided_split: rows [*split_row0, *split_row0 + *split_rows)).  ksize 15: every row of the frame, one launch (the
 * kernel reflects row indices at the top and bottom borders itself).  ksize 10 / 20 (non-symmetric window): the whole
 * ring periods between row ksize and row H - (ksize - 2); the rows above and below go to the general kernel
 * (k_guided_pipe) in a second launch.  0 rows = the general kernel alone (small jobs, odd widths, other windows).
 * For benchmarks that price each kernel by the pixels it covers.  The function has no context: it answers for the DEFAULT
 * tuning (gf_split = 1, gf_bands = 0); a context with other settings runs a different plan. */
int uwie_guided_plan(int batch, int H, int W, int ksize, int *split_row0, int *split_rows);

/* The strip-wavefronts of that plan: strips x bands x batch, 0 where uwie_guided_plan answers 0 rows.  A strip-wavefront is
 * one wavefront that filters one band of one 100-column strip (ksize 15); a compute unit holds eight at a time.  Tuning
 * gf_fuse = 2 holds this number against the device's compute units x 8 (see uwie_set_tuning).  No context, as above. */
int uwie_guided_fill(int batch, int H, int W, int ksize, long long *items);

/* How the CLAHE tail of a call is launched: the fused tail of strategies 1-2 (k_stretch_lab_lut<0|1> + k_clahe_apply_u8 /
 * k_clahe_apply_f32) and the code-domain tail of strategies 4-6 and dict clahe_enhancement (k_stretch_lab_lut<2> +
 * k_clahe_apply_codes).  The launchers themselves run on this plan, so a test can ask which route a shape takes.
 *   tile_w, tile_h   tile size on the frame as OpenCV pads it (both directions as soon as either is ragged: `padded`)
 *   clip_limit       the integer limit max(int(clip_limit * tile area / 256), 1); 0 for clip_limit <= 0 (no clipping)
 *   wide_lut         1: the 1024-thread LUT kernel (k_stretch_lab_lut_wide).  Only a recomputed source has it
 *                    (`recomputed` != 0: strategies 1-2 without uwie_set_tuning restore_store); few, large tiles
 *   nchunk           row chunks per interpolation cell of the apply kernel: its grid is (tiles_x+1)(tiles_y+1) nchunk x batch
 *   cells_walk       interpolation cells that hold pixels and whose blocks walk down the rows of fixed 4-pixel columns
 *   cells_flat       ... and whose blocks take the flat loop over all 4-pixel groups (cells wider than 1024 px, or of a
 *                    width that would leave more than an eighth of a column-walking block idle)
 * No context, as above: nothing here depends on a tuning. */
typedef struct uwie_clahe_plan_info {
    int32_t tile_w, tile_h, padded, clip_limit, wide_lut, nchunk, cells_walk, cells_flat;
} uwie_clahe_plan_info;
int uwie_clahe_plan(int batch, int H, int W, int tiles_x, int tiles_y, double clip_limit, int recomputed,
                    uwie_clahe_plan_info *out);

/* restore_image (S6:183-188): float32 [batch][H][W][3]. */
int uwie_restore(uwie_ctx *ctx, const uint8_t *d_in, const int32_t *d_kind, const float *d_A, const double *d_t,
                 int batch, int H, int W, float *d_out_f32, void *stream);

/* np.percentile(img[:,:,c], q) for every image, channel and q (NumPy 2.2.6 float32 arithmetic,
 * S6:196-197,216-217): d_out [batch][3][nq] float32.  q in percent. */
int uwie_percentiles_f32(uwie_ctx *ctx, const float *d_img, int batch, int H, int W, const double *q_percent, int nq,
                         float *d_out, void *d_workspace, size_t workspace_bytes, void *stream);

/* The same on float64 images [batch][H][W][3] (NumPy's float64 arithmetic, ES:265-266): d_out [batch][3][nq] float64. */
int uwie_percentiles_f64(uwie_ctx *ctx, const double *d_img, int batch, int H, int W, const double *q_percent, int nq,
                         double *d_out, void *d_workspace, size_t workspace_bytes, void *stream);

/* enhance_contrast / white_balance (S6:191-199, 211-219): clip((x-lo)/(hi-lo+1e-6),0,1). */
int uwie_stretch_f32(uwie_ctx *ctx, const float *d_img, float *d_out, int batch, int H, int W, double lo_percent,
                     double hi_percent, void *d_workspace, size_t workspace_bytes, void *stream);

/* gamma_correction: mode 1 = x**g (S6:222-224), mode 2 = clip(x**(1/g),0,1) (ES:276-285). */
int uwie_gamma_f32(uwie_ctx *ctx, const float *d_img, float *d_out, size_t n, double g, int mode, void *stream);

/* apply_clahe (S6:202-208): (x*255).astype(u8) -> RGB2LAB -> CLAHE(L) -> LAB2RGB -> /255 float32. */
int uwie_clahe_f32(uwie_ctx *ctx, const float *d_img, float *d_out, int batch, int H, int W, double clip_limit,
                   int tiles_x, int tiles_y, void *d_workspace, size_t workspace_bytes, void *stream);

/* the OpenCV primitives on their own (u8 in, u8 out) */
int uwie_rgb2gray_u8(uwie_ctx *ctx, const uint8_t *d_rgb, uint8_t *d_gray, size_t npixels, int gray_shift,
                     void *stream);
int uwie_rgb2lab_u8(uwie_ctx *ctx, const uint8_t *d_rgb, uint8_t *d_lab, size_t npixels, void *stream);
int uwie_lab2rgb_u8(uwie_ctx *ctx, const uint8_t *d_lab, uint8_t *d_rgb, size_t npixels, void *stream);
int uwie_clahe_u8(uwie_ctx *ctx, const uint8_t *d_plane, uint8_t *d_out, int batch, int H, int W, double clip_limit,
                  int tiles_x, int tiles_y, void *d_workspace, size_t workspace_bytes, void *stream);
/* cv2.Canny(gray, low, high) (S6:150): edge map (0/255) [batch][H][W]. */
int uwie_canny_u8(uwie_ctx *ctx, const uint8_t *d_gray, uint8_t *d_edges, int batch, int H, int W, int low, int high,
                  void *d_workspace, size_t workspace_bytes, void *stream);
/* cv2.equalizeHist per plane (ES:343): [batch][H][W]. */
int uwie_equalize_hist_u8(uwie_ctx *ctx, const uint8_t *d_plane, uint8_t *d_out, int batch, int H, int W,
                          void *d_workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* UWIE_H_ */
