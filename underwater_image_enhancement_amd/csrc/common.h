// Shared declarations of libuwie.so (gfx950 only; no CPU fallback anywhere in this library).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/uwie.h"

namespace uwie {

// ---------------------------------------------------------------- errors
void set_error(const char *fmt, ...);
#define UWIE_HIP_CHECK(expr)                                                            \
    do {                                                                                \
        hipError_t _e = (expr);                                                         \
        if (_e != hipSuccess) {                                                         \
            ::uwie::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return UWIE_E_HIP;                                                          \
        }                                                                               \
    } while (0)
#define UWIE_LAUNCH_CHECK() UWIE_HIP_CHECK(hipGetLastError())
#define UWIE_REQUIRE(cond, msg)                 \
    do {                                        \
        if (!(cond)) {                          \
            ::uwie::set_error("%s", msg);       \
            return UWIE_E_INVALID;              \
        }                                       \
    } while (0)

// ---------------------------------------------------------------- constant tables (device copies owned by the context)
constexpr int kCastBinadeMin = -2;  // sequential-mean emulation handles accumulators >= 2^-2 in closed form
constexpr int kCastBinades = 34;    // e = -2 .. 31

struct LabTables {           // OpenCV's integer sRGB<->Lab tables (see tables.cpp)
    uint16_t gamma[256];     // sRGBGammaTab_b
    uint16_t cbrt[3072];     // LabCbrtTab_b
    int32_t fwd[9];          // RGB->XYZ/white, 12-bit
    uint8_t invgamma[4096];  // sRGBInvGammaTab_b (values <= 255)
    int32_t ltoyf[512];      // LabToYF_b
    int32_t abtoxz[36864];   // abToXZ_b
    int32_t inv[9];          // XYZ*white->RGB, 12-bit
};

struct CastTables {                         // rounding tables for the sequential float32 mean (k_entry.hip)
    uint32_t R[kCastBinades][256];          // RN(x_k / ulp_e)
    uint8_t tie[kCastBinades][256];         // 1 if x_k / ulp_e has fractional part exactly 1/2
    uint32_t RT[256][kCastBinades];         // R transposed, tie in bit 31 (R < 2^26): one coalesced row per value
    uint2 RT2[128][kCastBinades];           // values 2j, 2j+1: x = low 13 bits of R as a 16-bit pair, y = R >> 13 likewise
    uint8_t tiebin[256];                    // the one binade index in which value k ties (255: none in range)
};

void build_lab_tables(LabTables *t);
void build_cast_tables(CastTables *t);

// ---------------------------------------------------------------- optional per-kernel timing (prof.hip)
struct Profiler;
Profiler *prof_create();
void prof_destroy(Profiler *p);
void prof_enable(Profiler *p, bool on);
void prof_filter(Profiler *p, const char *name);
void prof_bind(Profiler *p);  // makes p the recorder of this host thread (nullptr / disabled = no recording)
int prof_collect(Profiler *p);
int prof_row(Profiler *p, int i, const char **name, double *ms, int *calls);
class ProfScope {  // records a start event now and a stop event when it goes out of scope
public:
    ProfScope(const char *name, hipStream_t st);
    ~ProfScope();
    ProfScope(const ProfScope &) = delete;

private:
    int rec_;
    hipStream_t st_;
};
#define UWIE_PROF_CAT2(a, b) a##b
#define UWIE_PROF_CAT(a, b) UWIE_PROF_CAT2(a, b)
#define UWIE_PROF(name, st) ::uwie::ProfScope UWIE_PROF_CAT(_uwie_prof_, __LINE__)(name, st)
// every kernel launch goes through this: named timing scope + launch.  The profiler row is the kernel as written at the
// launch; UWIE_LAUNCH_AS names the row itself (a launch inside a template would report its parameter, not the type)
#define UWIE_LAUNCH_AS(row, kernel, grid, block, lds, st, ...)              \
    do {                                                                    \
        UWIE_PROF(row, st);                                                 \
        hipLaunchKernelGGL(kernel, grid, block, lds, st, __VA_ARGS__);      \
    } while (0)
#define UWIE_LAUNCH(kernel, ...) UWIE_LAUNCH_AS(#kernel, kernel, __VA_ARGS__)

}  // namespace uwie

namespace uwie {
// Route selectors of one context.  The defaults are what ships and what uwie_params cannot express: which of several
// equivalent routes a stage takes (tests force the fallback routes through uwie_set_tuning; profiles/ scripts compare
// them).  Environment variables UWIE_<NAME> are read ONCE, in uwie_create -- never per call.
struct Tuning {
    int gf_split = 1;           // guided filter: the split-ring wavefront kernel for large jobs (0: the general kernel alone)
    int gf_bands = 0;           // ... bands per strip (0: chosen from the job's size)
    int select_generic = 0;     // percentile selection: the three-digit key sweeps alone
    int restore_store = 0;      // strategies 1-2 / dict dehazing: keep the restored image in planes instead of recomputing it
    int lin_predict3 = 0;       // strategy 3: predicted windows as for strategies 1-2
    int lin_cap = 0;            // candidate list capacity (0: default; small values force the overflow fallback)
    int lin_no_predict = 0;     // no predicted windows: always the collecting sweep
    int q_hist = 1;             // quadtree levels decided from byte histograms when the interval test allows (2: never allows)
    int lin_predict_shift = 0;  // predicted windows moved by this many bins (large: every prediction misses)
    int streams = 1;            // uwie_enhance_u8: sub-batches on this many internal streams (1 .. 4)
    int canny_prepass = 1;      // quadtree: the streaming "any strong pixel?" pass before Canny
    int gf_fuse = 2;            // ... with t0 computed from the frame's bytes inside it (k_guided_split8, no k_trans_init and no t0 plane).  0: never;
                                // 1: whenever eligible; 2: auto -- eligible jobs of at least kFuseRounds rounds of the chip's resident
                                // strip-wavefronts (plan_guided; 4K x 64: 8.99 - 9.04 ms per step against 9.29 - 9.38)
    int rank_sweep = 1;         // strategies 1-2: the rank-counting restore sweep on jobs of >= 16 MP (0: the histogram sweep; 2: any size)
    int canny_fault_inject = 0; // tests only: k_canny_gradnms leaves out the root labels (the round-3 defect): uwie_device_status must report it
    int entry_fuse = 1;         // frames with W % 8 == 0: the level-0 quadrant histograms come out of cast detection's chunk pass and the
                                // gray plane out of the Canny pre-pass (0: k_q_hist<gray> + k_canny_strong as in rounds 3 - 4)
};
const Tuning &tune();  // tuning of the context whose entry point is running on this host thread (defaults outside one)
uwie_ctx *current_ctx();
}  // namespace uwie

struct uwie_ctx {
    int device;
    uwie::Tuning tune;
    bool attr_q_tail = false;   // > 64 KB LDS attributes set on this context's device: k_q_tail,
    bool attr_cast_resolve = false;  // k_cast_resolve (the rounding table of every binade: 70 KB),
    int attr_gf_fast = 0;       // k_guided_fast<TH> (bit TH)
    int attr_gf_split8 = 0;     // k_guided_split8<15, double / float> (bits 1 / 2)
    int cus = 0;                // compute units of the device (uwie_create): what "the job fills the chip" is measured against
    uwie::LabTables *d_lab;
    uwie::CastTables *d_cast;
    uwie::Profiler *prof;
    uint32_t *d_status = nullptr;  // device status word: UWIE_STATUS_* bits set by kernels that find an invariant violated
    // two-way batch pipelining (uwie_enhance_u8): helper streams and the fork / join events, created on first use
    hipStream_t aux[4];
    hipEvent_t fork, join[4];
    bool aux_ready;
    // the last enhance call on this context was uwie_enhance_u8_f64, which never splits the batch (uwie_enhance_percentiles)
    bool last_enhance_f64 = false;
};

namespace uwie {

// ---------------------------------------------------------------- workspace carving
struct Carver {
    char *base;
    size_t off;
    explicit Carver(void *b) : base(static_cast<char *>(b)), off(0) {}
    template <typename T>
    T *take(size_t count)
    {
        off = (off + 255) & ~size_t(255);
        T *p = base ? reinterpret_cast<T *>(base + off) : nullptr;
        off += count * sizeof(T);
        return p;
    }
    size_t total() const { return (off + 255) & ~size_t(255); }
};

static inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }
// blocks of 256 threads for a grid-stride loop over n items
static inline int grid_for(size_t n, size_t cap = 8192)
{
    size_t g = (n + 255) / 256;
    if (g > cap) g = cap;
    return g < 1 ? 1 : (int)g;
}

// ---------------------------------------------------------------- region descriptor used by the Canny / quadtree kernels
struct Region {  // a rectangle of image `img`; rows == 0 marks an inactive region
    int32_t img, y0, x0, rows, cols;
};

// ---------------------------------------------------------------- stage launchers (each enqueues on `stream`, returns UWIE_*)
struct Shape {
    int B, H, W;
    size_t npx() const { return (size_t)H * W; }
};

// k_entry.hip
size_t cast_ws_bytes(Shape s);
struct EntryFuse {       // what cast detection's chunk pass leaves for the quadtree (tuning entry_fuse)
    uint32_t *qpart;     // the level-0 quadrants' shares of every chunk
    uint8_t *gray;       // the gray plane, or nullptr (then the quadtree's level 0 writes it: k_gray_strong)
    int32_t *guess;      // [B] the cast kinds the plane was first written for
    int gray_shift;
};
int launch_cast_classify(uwie_ctx *ctx, const uint8_t *d_in, Shape s, int32_t *d_kind, float *d_mean, void *ws,
                         hipStream_t st, const EntryFuse *ef = nullptr);
size_t quad_part_bytes(Shape s);  // the level-0 quadrants' shares of every chunk (tuning entry_fuse)
int launch_quad_hist_reduce(const uint32_t *qpart, Shape s, uint32_t *d_hist, hipStream_t st);
int launch_set_kind(int32_t *d_kind, int B, int kind, hipStream_t st);
int launch_normalise_correct(const uint8_t *d_in, const int32_t *d_kind, float *d_out, Shape s, hipStream_t st);
int launch_quant_gray(const uint8_t *d_in, const int32_t *d_kind, uint8_t *d_gray, Shape s, int gray_shift,
                      hipStream_t st);

// k_airlight.hip
size_t airlight_ws_bytes(Shape s);
// make_gray_shift != 0: d_gray is written on the way (the level-0 sums pass or k_quant_gray) instead of read
// qpart: the level-0 quadrant shares that launch_cast_classify left for these frames (entry_fuse_takes), or nullptr
int launch_airlight(uwie_ctx *ctx, const uint8_t *d_in, const int32_t *d_kind, uint8_t *d_gray, Shape s, int min_size,
                    float *d_A, void *d_trace, void *ws, hipStream_t st, int make_gray_shift = 0, const uint32_t *qpart = nullptr);
bool entry_fuse_takes(Shape s, int min_size);

// k_canny.hip  (regions: device array of nreg Region; max_rows/max_cols bound every region)
size_t canny_ws_bytes(Shape s);
int launch_canny(const uint8_t *d_gray, Shape s, const Region *d_regions, int nreg, int max_rows, int max_cols, int low,
                 int high, uint32_t *d_count, uint8_t *d_edges, void *ws, hipStream_t st, bool count_is_zeroed = false,
                 bool strong_is_zeroed = false, bool prepass_done = false);
bool gray_strong_takes(Shape s);
int launch_gray_strong(const uint8_t *d_in, const int32_t *d_kind, uint8_t *d_gray, Shape s, const Region *d_regions, int nreg,
                       int max_rows, int max_cols, int high, int gray_shift, void *ws, hipStream_t st);
int launch_hist_strong(const uint8_t *d_in, const uint8_t *d_gray, Shape s, const Region *d_regions, int nreg, int max_rows,
                       int max_cols, int high, uint32_t *d_hist, void *ws, hipStream_t st);
uint32_t *canny_strong_flags(void *ws, Shape s);  // the pre-pass flags inside a Canny workspace ([regions])
int launch_make_full_regions(Region *d_regions, Shape s, hipStream_t st);

// k_airlight.hip: NumPy-order sum / mean / sum of squared deviations per region and channel
int launch_region_stats(const uint8_t *d_in, const int32_t *d_kind, const Region *d_regs, int nreg, int max_rows,
                        int max_cols, Shape s, float *csum, int maxChunks, float *tot, float *mean, float *vtot,
                        hipStream_t st);
// k_codes.hip: hist[b][c][256] += counts of the u8 frame (caller zeroes)
int launch_frame_hist(const uint8_t *d_in, Shape s, uint32_t *d_hist, hipStream_t st);
// k_features.hip: vgg_16_UIE.extract_all_features (79 floats per image)
size_t features_ws_bytes(Shape s);
int launch_features_u8(const uint8_t *d_in, Shape s, float *d_out, void *ws, hipStream_t st);

// k_quality.hip: quality_assessment.QualityAssessment scores, [B][9] float64 (8 scores + weighted total)
size_t quality_ws_bytes(Shape s);
int launch_quality_scores(uwie_ctx *ctx, const uint8_t *d_u8, const float *d_f32, Shape s, int gray_shift,
                          const double *weights8, double *d_scores, void *ws, hipStream_t st);

// k_extractor.hip: feature_extraction.FeatureExtractor.extract_all_features, [B][79] float64 ([B][74]: odd dimension > 1, no DCT)
bool feature_extractor_has_dct(int H, int W);
int feature_extractor_count(int H, int W);
size_t feature_extractor_ws_bytes(Shape s);
int launch_feature_extractor(uwie_ctx *ctx, const uint8_t *d_u8, const float *d_f32, Shape s, int gray_shift, double *d_out,
                             void *ws, hipStream_t st);

// k_resize.hip: cv2.resize of a ragged batch of RGB u8 frames (device descriptor table), u8 / float32 / normalised outputs
int launch_resize_rgb(const uwie_frame_desc *d_desc, int B, int oh, int ow, const uint8_t *d_flips, uint8_t *d_u8, float *d_f32,
                      float *d_norm, const float *mean3, const float *std3, uint32_t *d_status, hipStream_t st);

// k_classify.hip: scaler + RandomForest / GradientBoosting / SVC(rbf) prediction per row (main.py:398-433)
struct ClsNode {  // one tree node; a leaf has left = right = -1 (its feature is 0)
    double thr;
    int32_t left, right, feat, miss;
};
struct ClsModel {  // device pointers into one blob (uwie_model_create)
    int kind, F, C, T, K, S;
    double lr, gamma;
    const double *mean, *scale;
    const int32_t *tree_off;  // [T + 1]
    const ClsNode *nodes;     // [N]
    const double *value;      // RF [N][C], GB [N]
    const double *init;       // GB [K]
    const double *svT;        // SVC [F][S]: support vectors, feature-major
    const double *coef;       // [C - 1][S]
    const double *rho;        // [P] = -intercept
    const double *prob_a, *prob_b;
    const int32_t *sv_start;  // [C + 1]
};
int classify_model_check(const uwie_model_desc *d);
size_t classify_blob_bytes(const uwie_model_desc *d);
ClsModel classify_pack(const uwie_model_desc *d, void *host_blob, const void *dev_blob);
int launch_classify(const ClsModel &m, const double *d_rows, int B, int32_t *d_label, double *d_proba, uint32_t *d_status,
                    hipStream_t st);

// best[b] = first argmax over the n sets of scores[k][b][col] (rows of ncols); d_out (optional) [B][H][W][3] = d_all[best[b]][b]
int launch_pick_best(const double *d_scores, int n, Shape s, int ncols, int col, const uint8_t *d_all, int32_t *d_best, uint8_t *d_out,
                     hipStream_t st);

// k_uw_quality.hip: UCIQE / UIQM and their parts (include/uwie.h uwie_underwater_scores_u8), [B][kUwScores] float64
constexpr int kUwScores = UWIE_UW_SCORES;
size_t underwater_ws_bytes(Shape s);
void underwater_tile(int *tile_w, int *tile_h);  // the tile of one block of the block pass (uwie_underwater_plan)
int launch_underwater_scores(uwie_ctx *ctx, const uint8_t *d_u8, Shape s, int gray_shift, double *d_scores, void *ws, hipStream_t st);

// k_ref_quality.hip: MAE, MSE, PSNR and SSIM against a reference (include/uwie.h uwie_reference_scores_u8), [B][kRefScores]
// float64; frame i is compared with reference i % ref_batch
constexpr int kRefScores = UWIE_REF_SCORES;
size_t reference_ws_bytes(Shape s);
void reference_tile(int *tile_w, int *tile_h);  // the map points of one workgroup of the SSIM pass (uwie_reference_plan)
int launch_reference_scores(const uint8_t *d_u8, const uint8_t *d_ref_u8, Shape s, int ref_batch, int gray_shift, double *d_scores,
                            void *ws, hipStream_t st);

// k_gray_world.hip: gray-world white balance with red-channel compensation (include/uwie.h uwie_gray_world_u8); d_out / d_stats
// optional (at least one), d_out == d_in allowed, ws: gray_world_ws_bytes
size_t gray_world_ws_bytes(Shape s);
void gray_world_plan(int *block_px, int *thread_px);  // pixels per workgroup of the sum pass, per thread of the apply pass
int launch_gray_world(const uint8_t *d_in, Shape s, double red, double blue, double max_gain, uint8_t *d_out, double *d_stats, void *ws,
                      hipStream_t st);

// k_fusion.hip: multi-scale fusion of a gamma-corrected and a sharpened input (include/uwie.h uwie_fusion_u8); d_in1 / d_in2 /
// d_weight optional, ws: fusion_ws_bytes
size_t fusion_ws_bytes(Shape s, int levels);
void fusion_tile(int *tile_w, int *tile_h);             // the level-0 tile one workgroup stages with its halo
void fusion_table(double gamma, uint8_t *table256);     // G of the contract, on the host
int launch_fusion(const uint8_t *d_in, Shape s, double gamma, int levels, int gray_shift, uint8_t *d_out, uint8_t *d_in1, uint8_t *d_in2,
                  double *d_weight, void *ws, hipStream_t st);

// k_guided.hip
size_t guided_ws_bytes(Shape s);
size_t box_ws_bytes(Shape s);
int launch_trans_init(const uint8_t *d_in, const int32_t *d_kind, const float *d_A, Shape s, float omega, float norm_eps,
                      int pre_clip, float *d_t0, hipStream_t st);
int launch_box_filter_f64(const double *d_src, double *d_dst, Shape s, int k, void *ws, hipStream_t st);
// k_dark_patch.hip: t0 with the dark channel taken over a k x k patch (uwie_params.dark_patch = k, 2 .. 31): cv2.erode's
// rectangle, centre anchor and border between the channel minimum and 1 - omega * dark.  One launch, no workspace.
int launch_trans_patch(const uint8_t *d_in, const int32_t *d_kind, const float *d_A, Shape s, int k, float omega, float norm_eps,
                       int pre_clip, float *d_t0, hipStream_t st);
void dark_patch_tile(int *tile_w, int *tile_h);  // the output tile of one block (uwie_dark_patch_plan)
int launch_guided(const uint8_t *d_gray, const float *d_t0, Shape s, int k, double eps, double *d_t, void *ws,
                  hipStream_t st);
int launch_guided_p64(const uint8_t *d_gray, const double *d_t0, Shape s, int k, double eps, double *d_t, void *ws, hipStream_t st);

// The guided filter's routes (k_guided_pipe.hip): plan_guided is the one place that decides which kernels filter a job,
// what they need of the workspace and how t comes out; launch_guided_plan runs a plan and never declines one.
enum GuidedRoute {
    GF_EXACT,  // k_guided.hip: cv2.boxFilter's summation order, six float64 planes of workspace (guided_ws_bytes)
    GF_FAST,   // k_guided_fast<TH>: LDS strips (windows and frames the wavefront kernels do not take)
    GF_PIPE,   // k_guided_pipe: the general wavefront kernel, float64 or fixed-point a/b ring
    GF_SPLIT,  // k_guided_split (+ a k_guided_pipe border launch for even windows): large jobs
    GF_FUSED,  // k_guided_split8: GF_SPLIT with t0 computed from the frame inside it (tuning gf_fuse: chip-filling jobs by default)
};
struct GuidedRequest {
    int k;
    double eps;
    bool exact = false;          // cv2.boxFilter's summation order (uwie_params.gf_exact)
    bool fx = false;             // fixed-point a/b ring wanted; the caller guarantees 0.1 <= t0 <= 1 (pre-clipped transmission)
    bool f32_ok = false;         // t may be written as float32
    bool t0_from_frame = false;  // t0 may be computed from the u8 frame inside the filter
    bool t0_f64 = false;         // t0 is float64: the exact-order kernels only
};
struct GuidedPlan {
    GuidedRoute route;
    int k;
    double eps;
    bool t_f32;    // t is written as float32
    bool ring_fx;  // GF_PIPE: fixed-point a/b ring
    bool t0_f64;   // GF_EXACT: float64 t0
    bool t0;       // a t0 plane is read (every route but GF_FUSED)
    bool planes;   // the six float64 planes are needed (GF_EXACT): depends on the request and the shape, never on tuning
    int TH;        // GF_FAST: rows per step
    int iy0, band, nb, rows;  // GF_SPLIT / GF_FUSED: rows [iy0, iy0 + rows) in nb bands of `band` rows
    int pipe_bands;           // GF_PIPE and GF_SPLIT's border launch: bands per strip of the general kernel
};
GuidedPlan plan_guided(Shape s, const GuidedRequest &r);
// strip-wavefronts of a split plan (strips x bands x images): what tuning gf_fuse = 2 holds against the chip's resident set
inline long long guided_items(Shape s, const GuidedPlan &g) { return (long long)cdiv(s.W, 128 - 2 * (g.k - 1)) * g.nb * s.B; }
// t0 from the u8 frame: 1 - omega * min_c(img / (A + norm_eps)), clipped to [0.1, 1] with pre_clip (k_trans_init)
struct FuseT0Args {
    const uint8_t *rgb;    // [B][H][W][3]
    const int32_t *kind;   // [B] cast kinds or nullptr
    const float *A;        // [B][3]
    float omega, norm_eps;
    int pre_clip;
};
// d_t0: float32 (float64 for t0_f64 plans), not read by GF_FUSED, which computes it from *frame; d_t: float64, or float32
// data for t_f32 plans; ws: the six planes of GF_EXACT
int launch_guided_plan(const GuidedPlan &g, Shape s, const uint8_t *d_gray, const void *d_t0, double *d_t, void *ws, hipStream_t st,
                       const FuseT0Args *frame = nullptr);
// k_guided_fast.hip: the rows per step (8, 4, 2) of the k_guided_fast<TH> kernel that takes this job, 0 = none
int guided_fast_th(Shape s, int k);
int launch_guided_fast(const uint8_t *d_gray, const float *d_t0, Shape s, int k, int TH, double eps, double *d_t, hipStream_t st);

// k_select.hip
constexpr int kMaxPct = 4;  // percentiles per call
size_t select_ws_bytes(Shape s);
// The selection's host entry points are templates on the value type V = float (S6 surface) or double (ES surface), defined
// and instantiated for both in k_select.hip.
// d_vals: image of V, HWC ([B][H][W][3], planar = 0) or planar ([B][3][H][W], planar = 1); d_out [B][3][nq]
template <typename V>
int launch_percentiles(const V *d_vals, int planar, Shape s, const double *q_percent, int nq, V *d_out, void *ws, hipStream_t st);
// d_out[i] = (double)d_in[i], i < n
int launch_widen_f32(const float *d_in, double *d_out, size_t n, hipStream_t st);

// selection in pieces, for producers that fuse the first histogram sweep (digit = f32_key(v) >> 21 resp. f64_key(v) >> 53,
// 2048 bins, accumulated into plan.ghist[(b*3 + c) * kSelGroupStride + digit])
constexpr int kSelGroupStride = 2 * kMaxPct * 2048;
constexpr int kSelOsStride = 2 * kMaxPct;  // order statistics per (image, channel) in SelectPlan::os
struct LinState;
struct SelectPlan {
    void *state;
    uint32_t *ghist;
    void *os;              // order statistics, float or double [B*3][8]
    double t[kMaxPct];     // lerp weights (exactly representable values of the data's dtype)
    int nq;
    bool is64;
    // linear-digit path (select_lin_*): per (image, channel) state, candidate lists and fallback flags
    LinState *lin;
    void *lists;           // [B*3][kLinLists][cap] values of the data's dtype: read through lists_as
    uint32_t *flags;       // [B*3] 1 = a candidate list overflowed, use the key-digit passes
    uint32_t cap;
    bool predicted;        // the producer files the predicted windows: the collecting sweep is the rare fallback
    uint32_t ranks[2 * kMaxPct];
    template <typename V>
    V *lists_as() const { return static_cast<V *>(lists); }
};
// Selection on clipped [0, 1] float32 planes with ONE sweep after the producer's histogram: the first digit is a linear
// 2050-way split of [0, 1] (exact 0 and exact 1 get their own bins), which a whole frame spreads over thousands of bins,
// so the elements of the few target bins are collected during the sweep and the rest of the selection runs on those
// short lists.  lin_digit() is the split; the producer adds its counts to plan.ghist[(b*3+c)*kSelGroupStride + digit].
constexpr int kLinBins = 2050;
__host__ __device__ inline uint32_t lin_digit(float x)
{
    if (!(x > 0.0f)) return 0;          // zeros (and anything not above zero)
    if (x >= 1.0f) return kLinBins - 1;
    const uint32_t d = (uint32_t)(x * 2048.0f);  // exact product, truncation: monotone in x
    return 1 + (d > 2047u ? 2047u : d);
}
__host__ __device__ inline uint32_t lin_digit(double x)  // the same split for the float64 planes of the ES surface
{
    if (!(x > 0.0)) return 0;
    if (x >= 1.0) return kLinBins - 1;
    const uint32_t d = (uint32_t)(x * 2048.0);
    return 1 + (d > 2047u ? 2047u : d);
}
// Per (image, channel) state of the linear-digit selection.  With a prediction (select_lin_begin<V>(..., predict)) the
// producer already files the elements of two windows of bins, each around the predicted position of a percentile's
// ranks, into one list per window during its own sweep; the scan then checks the prediction against the exact
// histogram, and only planes it missed need the collecting sweep (whose groups reuse the lists).
constexpr int kLinLists = 2 * kMaxPct;   // candidate lists per (image, channel)
constexpr uint32_t kLinNoWin = 0x80000000u;
struct LinState {
    uint32_t rr[2 * kMaxPct];    // rank of the query inside its bin
    uint32_t qbin[2 * kMaxPct];  // bin of the query
    uint32_t gid[2 * kMaxPct];   // list of the query; kLinDone: answered by the scan
    uint32_t gbin[2 * kMaxPct];  // bin of the collecting sweep's group g (list g)
    uint32_t gcount[kLinLists];  // elements filed in each list
    uint32_t ngroups;            // groups the collecting sweep has to fill (0: the prediction covered every query)
    uint32_t wlo[kMaxPct], wspan[kMaxPct];  // predicted windows (one per percentile, merged when they touch): bins
                                            // wlo .. wlo + wspan (wlo = kLinNoWin: none), list = window
    uint32_t below[kMaxPct];     // (rank-counting sweep, k_restore_rank) elements in the bins below window w
};
// The rank route has two windows per plane, not kLinLists lists: the same memory as 2 lists of kRankCapMul x cap elements (a window
// of whole histogram bins holds 1 - 2 % of a plane whose values cluster on a few levels -- hazy noise frames: 139 K of 8.3 M -- and
// the histogram route's cap of 1/64 overflowed there on two planes in 192)
constexpr int kRankCapMul = 4;
constexpr uint32_t kLinAnyBin = 0xfffffffeu;  // LinState::qbin: the query's list is its whole window, rr its rank inside it
struct RestoreSrc;
// predict != nullptr: the target bins are predicted from a subsample of the restored image (k_lin_sample)
template <typename V>
int select_lin_begin(Shape s, const double *q_percent, int nq, void *ws, hipStream_t st, SelectPlan *plan,
                     const RestoreSrc *predict = nullptr);
// src != nullptr: the values are recomputed from *src (d_planar is not read); flagged planes take the key-digit passes
template <typename V>
int select_lin_run(const SelectPlan &plan, const V *d_planar, Shape s, hipStream_t st, const RestoreSrc *src = nullptr);
template <typename V>
int select_begin(Shape s, const double *q_percent, int nq, void *ws, hipStream_t st, SelectPlan *plan);
template <typename V>
int select_run(const SelectPlan &plan, const V *d_vals, int planar, Shape s, bool pass1_done, hipStream_t st);
template <typename V>
int select_lerp(const SelectPlan &plan, Shape s, V *d_out, hipStream_t st);                         // [B][3][nq]
int select_lerp_chain(const SelectPlan &plan, Shape s, float eps, float *d_pct4, hipStream_t st);   // [B][3][4]
// explicit sorted positions per image (vgg_16_UIE.py:78-82): os[bc*8 + 0/1] = sorted[int(L_low/100*n)], sorted[int(L_high/100*n)]
int select_begin_stretch_ranks(Shape s, const float *d_params, int stride, void *ws, hipStream_t st, SelectPlan *plan);
// the same with Python's indexing rules (deep_learning_parameters.py:73-77, devutil.h gated_rank): an image without a valid
// position selects position 0 and sets UWIE_STATUS_DIFF_RANK in *d_status
int select_begin_gated_ranks(Shape s, const float *d_params, int stride, uint32_t *d_status, void *ws, hipStream_t st,
                             SelectPlan *plan);
// k_diffenh.hip: DifferentiableEnhancement.forward (vgg_16_UIE.py:32-128) after the selection
// d_saved (optional): [B][3][2] float = {p_lo, p_hi} per plane, what the backward needs from the forward
int launch_diff_enhance(const float *d_img, int planar, Shape s, const float *d_params, int flags, const float *d_os,
                        float *d_out, hipStream_t st, float *d_saved = nullptr);
// k_diff_u8.hip: the same module from the frame's bytes (histogram -> the two bins -> per-block stretch tables -> apply);
// d_out_u8 / d_out_f32 / d_saved optional (at least one output), ws: diff_u8_ws_bytes
size_t diff_u8_ws_bytes(Shape s);
int launch_diff_enhance_u8(const uint8_t *d_in, Shape s, const float *d_params, int flags, uint8_t *d_out_u8, float *d_out_f32,
                           float *d_saved, void *ws, hipStream_t st);
// k_diff_u8.hip: the gated module for u8 frames in the byte domain: per image a 3 x 256 table.
// d_out_u8 / d_out_f32 / d_saved optional (at least one output), ws: diff_gated_u8_ws_bytes (independent of H x W)
size_t diff_gated_u8_ws_bytes(int B);
int launch_diff_gated_u8(const uint8_t *d_in, Shape s, const float *d_params, uint32_t *d_status, uint8_t *d_out_u8,
                         float *d_out_f32, float *d_saved, void *ws, hipStream_t st);
// k_diffenh.hip: deep_learning_parameters.DifferentiableEnhancement.forward (:32-55), the gated gamma module
// (params [B][4] = L_low, L_high, use_gamma, gamma; images without a valid sorted position get NaN)
int launch_diff_gated(const float *d_img, int planar, Shape s, const float *d_params, const float *d_os, float *d_out,
                      hipStream_t st, float *d_saved = nullptr);
// the gradient of either module, map = UWIE_LOSS_VGG / UWIE_LOSS_GATED (two launches: per-block partials, then a fixed-order
// finish and the sorted-position scatter).  With d_grad_loss the sweep adds ReferenceLoss's gradient against d_ref (below);
// without (nullptr, d_ref unused) it is the plain module backward of d_grad_out.
size_t diff_enhance_bwd_ws_bytes(Shape s);
int launch_module_bwd(int map, const float *d_img, int planar, Shape s, const float *d_params, int flags, const float *d_saved,
                      const float *d_ref, const float *d_grad_out, const float *d_grad_loss, float *d_grad_img,
                      float *d_grad_params, void *ws, hipStream_t st);
// k_diffenh.hip: ReferenceLoss (l1 = mean|o - r|, l2 = mean((o - r)^2)) fused into the module sweeps; map = UWIE_LOSS_*.
// Forward: after the selection (d_os; not read for the identity map), writes d_loss [2] and optionally d_out / d_saved.
// Backward: the module's backward with the loss gradient (d_grad_loss [2] on the device) in place of grad_out.
size_t refloss_ws_bytes(Shape s);
int launch_refloss(int map, const float *d_img, int planar, Shape s, const float *d_params, int flags, const float *d_os,
                   const float *d_ref, float *d_out, float *d_saved, float *d_loss, void *ws, hipStream_t st);
int launch_refloss_bwd(int map, const float *d_img, int planar, Shape s, const float *d_params, int flags, const float *d_saved,
                       const float *d_ref, const float *d_grad_out, const float *d_grad_loss, float *d_grad_img,
                       float *d_grad_params, void *ws, hipStream_t st);
// k_vgg.hip: PerceptualLoss, vgg16().features[:16].  A VggNet holds the packed weights of one
// precision (UWIE_VGG_F32 / UWIE_VGG_F16): w0 = conv1_1 [64][3][3][3] float32; for layers 1..6 wf [Cout][9][Cin] and the
// data-gradient's rotated wb [Cin][9][Cout] in the element type; bias [Cout] float32 for all seven.
struct VggNet {
    int precision;
    const float *w0;
    const void *wf[7], *wb[7];
    const float *bias[7];
};
size_t vgg_param_count();
size_t vgg_blob_bytes(int precision);
int vgg_pack(const float *d_params, int precision, void *blob, VggNet *net, hipStream_t st);
size_t perceptual_ws_bytes(Shape s, int precision);
int launch_perceptual(const VggNet &net, const float *d_pred, const float *d_target, Shape s, float *d_loss, void *ws, hipStream_t st);
int launch_perceptual_bwd(const VggNet &net, Shape s, const float *d_grad_loss, float *d_grad_pred, void *ws, hipStream_t st);
// k_vgg.hip: one more float32 3x3 conv packed as k_vgg_conv reads it (wf [Cout][9][Cin]; wb_scratch receives the rotated
// data-gradient copy, Cout * 9 * Cin floats, and may be freed after the stream has run)
int vgg_pack_conv_f32(const float *src, int Cout, int Cin, float *wf, float *wb_scratch, float *bias, hipStream_t st);
// k_vgg.hip: ImprovedVGGParameterNet's trunk, features[:23] in float32: conv1_1 ... relu3_3, pool3, conv4_1 ... relu4_3
// into X or Y (both B * H * W * 64 floats, used as a ping-pong); returns relu4_3's buffer [B][H/8][W/8][512]
int launch_param_trunk(const VggNet &net, const float *const wf4[3], const float *const bias4[3], const float *img, Shape s, float *X,
                       float *Y, float **relu43, hipStream_t st);
// k_param_net.hip: ImprovedVGGParameterNet
struct ParamNet {
    VggNet trunk;  // UWIE_VGG_F32, layers 0 .. 6
    const float *wf4[3], *bias4[3];
    int din;                           // 1103 (use_features) or 1024
    const float *lw[6], *lb[6];        // fusion.0, fusion.4, attention.0, attention.2, heads.0 (4 x 128 rows), heads.3 ([4][128])
    const float *bn[2];                // [4][C] = weight, bias, running_mean, running_var of fusion.1 / fusion.5
};
size_t param_net_count(int use_features);
size_t param_net_blob_bytes(int use_features);
int param_net_pack(const float *d_params, int use_features, void *blob, float *scratch, ParamNet *net, hipStream_t st);
size_t param_net_scratch_floats();
size_t param_net_ws_bytes(Shape s);
int launch_param_net(const ParamNet &net, const float *img, const float *feat, Shape s, float *out, float *pooled, void *ws,
                     hipStream_t st);
int launch_u8_to_f32(const uint8_t *d_in, size_t n, float *d_out, hipStream_t st);
// k_param_net.hip: deep_learning_parameters.ParameterPredictor in eval mode
struct Mlp {
    int F, H, nb;            // feature_dim, hidden_dim, num_blocks
    const float *base;       // input_proj.0 ... output_proj.0 in state_dict() order
    const float *hw, *hb;    // the four heads as one layer, [4][H / 2] and [4], in the gated order
};
size_t mlp_count(int F, int H, int nb);
int mlp_pack(const float *d_params, int F, int H, int nb, float *blob, Mlp *net, hipStream_t st);
size_t mlp_ws_bytes(int B, int hidden);
// feat: [B][F] float32, or float64 (f64) rounded to float32 on load; out: [B][4] = L_low, L_high, use_gamma, gamma
int launch_mlp(const Mlp &net, const void *feat, bool f64, int B, float *out, void *ws, hipStream_t st);
// k_mlp_train.hip: EndToEndTrainer's training step for ParameterPredictor.  Parameters, gradients and
// Adam's moments share mlp_pack's packed order.
struct MlpAdam {  // torch.optim.Adam's scalars for one step, rounded to float32 as torch's kernels take them
    float max_norm, w1, beta2, w2, bc2_sqrt, eps, neg_step;  // w1 = 1 - beta1, w2 = 1 - beta2, neg_step = -lr / (1 - beta1^t)
};
size_t mlp_train_ws_bytes(int B, int hidden, int nb);
int mlp_train_sites(int nb);
// given: uint8 [sites][B][H] or nullptr (drawn from seed, step); drawn_out: where the drawn masks go, or nullptr
int launch_mlp_train_forward(const Mlp &net, const void *feat, bool f64, int B, double p, const uint8_t *given, uint8_t *drawn_out,
                             uint64_t seed, uint32_t step, float *out, void *ws, hipStream_t st);
int launch_mlp_backward(const Mlp &net, float *grads, const void *feat, bool f64, int B, float scale, const float *grad_out, void *ws,
                        hipStream_t st);
size_t mlp_adam_scratch_bytes();
int launch_mlp_adam(const Mlp &net, float *params, float *grads, float *m, float *v, double *partial, const MlpAdam &h, double *norm_out,
                    hipStream_t st);
int mlp_repack(const float *src, float *dst, int F, int H, int nb, bool to_state, hipStream_t st);

// k_fused.hip: the fused tail of the dehazing strategies
// what the restored image (six_stadigy.py:183-188) is made of; consumers may recompute it from here (restore.h)
struct RestoreSrc {
    const uint8_t *in;    // [B][H][W][3]
    const int32_t *kind;  // [B] cast kinds or nullptr
    const float *A;       // [B][3]
    const double *t;      // [B][H][W]; float32 data when t32 is set (uwie_params.inter_dtype = UWIE_INTER_F32T)
    int t32 = 0;
};
// plan != nullptr: the linear-digit histogram goes to plan->ghist and the elements of the predicted windows to the lists
// t32: d_t holds float32 data (RestoreSrc::t32)
int launch_restore_planar_hist(const uint8_t *d_in, const int32_t *d_kind, const float *d_A, const double *d_t, Shape s,
                               float *d_planar, uint32_t *d_ghist, hipStream_t st, bool linear = false,
                               const SelectPlan *plan = nullptr, int t32 = 0);
// the rank-counting sweep (k_restore_rank): counts below each predicted window + the windows' members, no histogram
int launch_restore_rank(const RestoreSrc &src, Shape s, const SelectPlan &plan, hipStream_t st);
int select_rank_run(const SelectPlan &plan, Shape s, hipStream_t st, const RestoreSrc &src);
size_t tail_ws_bytes(Shape s, int tx, int ty);
// the launch plan of the CLAHE tail (uwie_clahe_plan): the same arithmetic the three launchers below run on
void clahe_plan_info(Shape s, double clip, int tx, int ty, bool recomputed, uwie_clahe_plan_info *out);
// d_pct: [B][3][pct_stride] = lo1, hi1 [, lo2, hi2]; two = second stretch present; gamma_mode 0/1/2
int launch_tail_clahe(uwie_ctx *ctx, const float *d_planar, const float *d_pct, int pct_stride, float eps, int two,
                      Shape s, double clip, int tx, int ty, int gamma_mode, double gamma, uint8_t *d_out_u8,
                      float *d_out_f32, void *ws, hipStream_t st, const RestoreSrc *src = nullptr);
int launch_codes_lab_lut(uwie_ctx *ctx, const uint8_t *d_in, const uint8_t *d_code_lut, Shape s, double clip, int tx, int ty,
                         uint8_t *d_lab, uint8_t *d_tile_lut, hipStream_t st);
int launch_clahe_apply_codes(uwie_ctx *ctx, const uint8_t *d_lab, const uint8_t *d_tile_lut, Shape s, double clip, int tx,
                             int ty, const uint8_t *d_fin_code, const float *d_fin_val, uint8_t *d_out_u8, float *d_out_f32,
                             uint8_t *d_codes_out, uint32_t *d_hist, hipStream_t st);
int launch_tail_plain(const float *d_planar, const float *d_pct, int pct_stride, float eps, int two, Shape s,
                      int gamma_mode, double gamma, uint8_t *d_out_u8, float *d_out_f32, hipStream_t st);
// ES surface (float64): recover_image (ES:237-249) -> planar float64 + first select digit; color_enhancement
// (ES:269-270, eps 1e-10) [-> gamma_correction (ES:284-285)] -> (y*255).astype(u8) (main.py:155) / float32 copy
int launch_recover64_planar_hist(const uint8_t *d_in, const float *d_A, const double *d_t, Shape s, double *d_planar,
                                 uint32_t *d_ghist, hipStream_t st, bool linear = false, const SelectPlan *plan = nullptr);
int launch_tail_plain64(const double *d_planar, const double *d_pct, Shape s, int apply_gamma, double gamma,
                        uint8_t *d_out_u8, float *d_out_f32, hipStream_t st, const RestoreSrc *src = nullptr,
                        double *d_out_f64 = nullptr);

// k_codes.hip: strategies 4-6 of six_stadigy.py and the clahe / histogram-equalisation strategies of
// enhancement_strategies.py, evaluated on 8-bit codes (per image and channel LUT chains + histograms)
size_t codes_ws_bytes(Shape s, int tx, int ty);
// quantised: d_in is (img * 255).astype(u8) of a general float image instead of the u8 frame the float image came from
int launch_code_strategy(uwie_ctx *ctx, const uint8_t *d_in, const int32_t *d_kind, Shape s, const uwie_params *p,
                         uint8_t *d_out_u8, float *d_out_f32, void *ws, hipStream_t st, double *d_out_f64 = nullptr,
                         bool quantised = false);

// k_float.hip: the front half of the strategies on general (not u8-derived) float images, T = float or double
size_t float_airlight_ws_bytes(Shape s);
template <class T> int launch_float_prepare(const T *d_x, const int32_t *d_kind, T *d_xc, uint8_t *d_q, Shape s, hipStream_t st);
template <class T> int launch_float_cast_classify(const T *d_x, Shape s, int32_t *d_kind, float *d_mean, hipStream_t st);
template <class T> int launch_float_airlight(const T *d_x, const uint8_t *d_gray, Shape s, int min_size, T *d_A, void *ws, hipStream_t st);
template <class T> int launch_float_trans_init(const T *d_x, const T *d_A, Shape s, double omega, double norm_eps, int pre_clip, T *d_t0,
                                               hipStream_t st);
template <class T, class OUT> int launch_float_restore(const T *d_x, const T *d_A, const double *d_t, Shape s, OUT *d_out, int planar,
                                                       hipStream_t st);

// k_tail.hip
int launch_restore(const uint8_t *d_in, const int32_t *d_kind, const float *d_A, const double *d_t, Shape s,
                   float *d_out, hipStream_t st);
// out = clip((x - lo) / (hi - lo + eps), 0, 1) with lo = d_pct[(b*3+c)*pct_stride + lo_idx], hi likewise
int launch_stretch_apply_f32(const float *d_img, const float *d_pct, int pct_stride, int lo_idx, int hi_idx, float eps,
                             float *d_out, Shape s, hipStream_t st);
int launch_gamma_f32(const float *d_img, float *d_out, size_t n, double g, int mode, hipStream_t st);
int launch_quantise_u8(const float *d_img, uint8_t *d_out, size_t n, hipStream_t st);

// k_clahe.hip
size_t clahe_ws_bytes(Shape s, int tx, int ty);
int launch_rgb2gray_u8(const uint8_t *d_rgb, uint8_t *d_gray, size_t n, int shift, hipStream_t st);
int launch_rgb2lab_u8(uwie_ctx *ctx, const uint8_t *d_rgb, uint8_t *d_lab, size_t n, hipStream_t st);
int launch_lab2rgb_u8(uwie_ctx *ctx, const uint8_t *d_lab, uint8_t *d_rgb, size_t n, hipStream_t st);
int launch_clahe_plane_u8(const uint8_t *d_plane, uint8_t *d_out, Shape s, double clip, int tx, int ty, void *ws,
                          hipStream_t st);
int launch_clahe_f32(uwie_ctx *ctx, const float *d_img, float *d_out, Shape s, double clip, int tx, int ty, void *ws,
                     hipStream_t st);
int launch_equalize_hist_u8(const uint8_t *d_plane, uint8_t *d_out, Shape s, void *ws, hipStream_t st);

}  // namespace uwie
