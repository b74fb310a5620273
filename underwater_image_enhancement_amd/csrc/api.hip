// C ABI of libuwie.so (include/uwie.h): context, parameter defaults, workspace sizing, the per-stage entry points
// and the strategy pipelines.  Everything here only enqueues kernels on the caller's stream.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <type_traits>

#include "common.h"

#include <cstdlib>

namespace uwie {

static thread_local char g_err[512] = "";
static thread_local uwie_ctx *g_ctx = nullptr;  // context of the entry point running on this thread
static const Tuning g_default_tuning{};

const Tuning &tune() { return g_ctx ? g_ctx->tune : g_default_tuning; }
uwie_ctx *current_ctx() { return g_ctx; }

void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

namespace {

// Every exported function that launches work runs inside one of these: the context's device becomes current (kernels,
// events and helper streams belong to it) and is put back afterwards, and the context's tuning is what tune() answers.
class CallScope {
public:
    explicit CallScope(uwie_ctx *ctx) : prev_ctx_(g_ctx)
    {
        g_ctx = ctx;
        if (ctx && hipGetDevice(&prev_dev_) == hipSuccess && prev_dev_ != ctx->device) {
            if (hipSetDevice(ctx->device) == hipSuccess) switched_ = true;
            else ok_ = false;
        }
    }
    ~CallScope()
    {
        if (switched_) (void)hipSetDevice(prev_dev_);
        g_ctx = prev_ctx_;
    }
    CallScope(const CallScope &) = delete;
    bool ok() const { return ok_; }

private:
    uwie_ctx *prev_ctx_;
    int prev_dev_ = -1;
    bool switched_ = false, ok_ = true;
};
#define UWIE_SCOPE(ctx)                                                       \
    CallScope _uwie_scope(ctx);                                               \
    if (!_uwie_scope.ok()) {                                                  \
        set_error("cannot make device %d current", (ctx)->device);           \
        return UWIE_E_HIP;                                                    \
    }

struct KnobName { const char *name; int Tuning::*field; };
const KnobName kKnobs[] = {{"gf_split", &Tuning::gf_split}, {"gf_bands", &Tuning::gf_bands},
                           {"select_generic", &Tuning::select_generic}, {"restore_store", &Tuning::restore_store},
                           {"lin_predict3", &Tuning::lin_predict3}, {"lin_cap", &Tuning::lin_cap},
                           {"lin_no_predict", &Tuning::lin_no_predict}, {"q_hist", &Tuning::q_hist}, {"lin_predict_shift", &Tuning::lin_predict_shift},
                           {"streams", &Tuning::streams}, {"canny_prepass", &Tuning::canny_prepass},
                           {"canny_fault_inject", &Tuning::canny_fault_inject}, {"rank_sweep", &Tuning::rank_sweep},
                           {"gf_fuse", &Tuning::gf_fuse}, {"entry_fuse", &Tuning::entry_fuse}};

void tuning_from_env(Tuning *t)  // uwie_create only
{
    for (const KnobName &k : kKnobs) {
        char var[64] = "UWIE_";
        size_t n = 5;
        for (const char *c = k.name; *c && n + 1 < sizeof var; ++c) var[n++] = (char)(*c >= 'a' && *c <= 'z' ? *c - 32 : *c);
        var[n] = 0;
        if (const char *e = getenv(var)) t->*(k.field) = atoi(e);
    }
}

bool shape_ok(int B, int H, int W)
{
    if (B < 1 || H < 1 || W < 1) return false;
    const long long npx = (long long)H * W;
    return npx < (1ll << 30) && (long long)B * npx < (1ll << 40);
}

#define UWIE_CHECK_SHAPE(B, H, W) UWIE_REQUIRE(shape_ok(B, H, W), "batch/H/W out of range")
#define UWIE_CHECK_WS(need)                                                                           \
    do {                                                                                              \
        if ((need) > 0 && (!d_workspace || workspace_bytes < (need))) {                               \
            set_error("workspace too small: need %zu bytes, got %zu", (size_t)(need), workspace_bytes); \
            return UWIE_E_WORKSPACE;                                                                  \
        }                                                                                             \
    } while (0)
#define UWIE_TRY(call)            \
    do {                          \
        int _rc = (call);         \
        if (_rc != UWIE_OK) return _rc; \
    } while (0)

// Buffers of one enhance() call, carved from the caller's workspace.
struct Pipe {
    int32_t *kind;
    float *A;
    float *pct;
    float *F;       // float32 working image (planar on the dehazing paths)
    double *F64;    // float64 planar image (dict-surface dehazing only)
    double *pct64;
    uint8_t *gray;
    float *t0;      // inside the scratch unless `planes`
    double *t;
    void *scratch;
    size_t scratch_bytes;
    bool planes;      // the scratch holds the exact-order guided filter's six float64 planes
    uint32_t *qpart;  // level-0 quadrant shares of cast detection's chunks (tuning entry_fuse; inside the scratch, behind what cast
                      // detection and the quadtree use), or nullptr
    int32_t *guess;   // ... and the cast kinds its gray plane was first written for
};

bool dehazes(const uwie_params *p)
{
    if (p->surface == UWIE_SURFACE_SIX) return p->strategy >= 1 && p->strategy <= 3;
    return p->strategy >= UWIE_DICT_STRONG_DEHAZING && p->strategy <= UWIE_DICT_LIGHT_ENHANCEMENT;
}

// uwie_params.dark_patch as the kernels take it: 0 means 1 (a zero-filled struct keeps the per-pixel dark channel)
int dark_patch_of(const uwie_params *p) { return p->dark_patch > 1 ? p->dark_patch : 1; }

// t0 of a u8 frame: the per-pixel dark channel (k_trans_init) or the one over a dark_patch x dark_patch window (k_trans_patch)
int launch_t0(const FuseT0Args &f, int patch, Shape s, float *d_t0, hipStream_t st)
{
    if (patch > 1) return launch_trans_patch(f.rgb, f.kind, f.A, s, patch, f.omega, f.norm_eps, f.pre_clip, d_t0, st);
    return launch_trans_init(f.rgb, f.kind, f.A, s, f.omega, f.norm_eps, f.pre_clip, d_t0, st);
}

// The plan of a u8 enhance call: plan_enhance is the one place that decides which pipeline runs a parameter set on a shape,
// which routes its stages take and what they need of the workspace; carve_pipe lays a plan out and run_enhance runs one, and
// neither decides anything.  tune() is read here (and in the planners this calls) and nowhere downstream: it is the calling
// context's tuning inside an entry point and the default tuning in uwie_workspace_bytes, which has no context --
// uwie_workspace_bytes_ctx answers for a context.
enum EnhancePipeline {
    EP_SIX_DEHAZE,   // six_stadigy strategies 1-3: cast, airlight, guided filter, restore, stretch, CLAHE / white balance
    EP_SIX_CODES,    // six_stadigy strategies 4-6: cast, then per-image LUT chains (k_codes.hip)
    EP_DICT_DEHAZE,  // strong / medium dehazing, light enhancement (ES:350-444) on the uncorrected frame
    EP_DICT_CODES,   // clahe_enhancement, histogram_equalization
};
struct EnhancePlan {
    EnhancePipeline pipeline;
    bool dehaze;        // a dehazing pipeline: gray plane, t0 and t exist
    GuidedPlan guided;  // ... and its guided filter, planned once: planes, t0 and t_f32 are read from here
    int dark_patch;     // t0 of the frame: the per-pixel dark channel (1, k_trans_init) or k_trans_patch's window
    // percentile selection and the restored image
    bool generic;   // the three- / six-digit key sweeps (tuning select_generic); otherwise the linear first digit (select_lin_*)
    bool store;     // the restored image is kept in planes; otherwise every sweep recomputes it from the frame and t
    bool predict;   // linear route: target windows predicted from a sample of the image
    bool rank;      // linear route: the rank-counting sweep (k_restore_rank) where the windows were predicted
    bool F, F64;    // which image planes the layout has (F64 comes with pct64)
    // cast detection's chunk pass feeding the quadtree (tuning entry_fuse)
    bool qpart;      // it leaves the level-0 quadrant histograms in the scratch, at qoff
    bool cast_gray;  // ... and writes the gray plane (entry_fuse = 2: the quadtree's pre-pass does, k_gray_strong)
    size_t qoff;
    int tx, ty;      // effective CLAHE tile grid
    size_t scratch_bytes;
    bool t0_in_scratch;
};

// The scratch of a layout: the largest share any of its stages takes.  The raw transmission lives from k_trans_init to the end
// of the guided filter; the scratch is idle exactly then (the quadtree is done with it, the selection has not started), so t0
// borrows its first 4 B/px -- unless the exact-order filter is on, whose six planes are IN the scratch while it reads t0.
// The quadrant histograms sit behind what cast detection and the quadtree use: they are written before the quadtree starts and
// read by its first launches.
void size_scratch(EnhancePlan &e, Shape s)
{
    const size_t none = 0, n = (size_t)s.B * s.npx();
    e.t0_in_scratch = e.dehaze && !e.guided.planes;
    e.scratch_bytes = std::max({cast_ws_bytes(s), e.dehaze ? airlight_ws_bytes(s) : none, e.guided.planes ? guided_ws_bytes(s) : none,
                                select_ws_bytes(s), clahe_ws_bytes(s, e.tx, e.ty), codes_ws_bytes(s, e.tx, e.ty),
                                e.t0_in_scratch ? n * sizeof(float) : none});
    e.qoff = e.qpart ? (std::max(cast_ws_bytes(s), airlight_ws_bytes(s)) + 255) & ~size_t(255) : 0;
    if (e.qpart) e.scratch_bytes = std::max(e.scratch_bytes, e.qoff + quad_part_bytes(s));
}

// p == NULL: any stage entry point (they carve their own, smaller layouts from the same buffer) -- the most demanding layout.
EnhancePlan plan_enhance(Shape s, const uwie_params *p)
{
    const Tuning &tu = tune();
    EnhancePlan e{};
    e.tx = p && p->tiles_x > 0 ? p->tiles_x : 8;
    e.ty = p && p->tiles_y > 0 ? p->tiles_y : 8;
    if (!p) {  // a dehazing call that stores float32 planes and filters in exact order
        e.pipeline = EP_SIX_DEHAZE;
        e.dehaze = e.store = e.F = e.guided.t0 = e.guided.planes = true;
        size_scratch(e, s);
        return e;
    }
    const bool six = p->surface == UWIE_SURFACE_SIX;
    e.dehaze = dehazes(p);
    e.pipeline = six ? (e.dehaze ? EP_SIX_DEHAZE : EP_SIX_CODES) : (e.dehaze ? EP_DICT_DEHAZE : EP_DICT_CODES);
    if (e.dehaze) {
        e.generic = tu.select_generic != 0;
        // The guided filter of a u8 call: t0 comes from the frame (k_trans_init / k_trans_patch, or inside the fused kernel).
        // The exact-order route materialises six float64 planes; the other routes keep everything on chip.
        GuidedRequest r{p->gf_ksize, p->gf_eps, p->gf_exact != 0};
        // fixed-point a/b ring: only with the pre-clipped transmission of the six_stadigy surface (0.1 <= t0 <= 1 bounds a, b)
        r.fx = six && p->inter_dtype == UWIE_INTER_FX32;
        // (the three-digit key sweeps of tuning select_generic instantiate the restore for the float64 plane only: no float32 t there)
        r.f32_ok = six && p->inter_dtype == UWIE_INTER_F32T && !e.generic;
        // a patched dark channel (dark_patch > 1) needs its neighbours' values: k_trans_patch writes the t0 plane, no route evaluates it
        e.dark_patch = dark_patch_of(p);
        r.t0_from_frame = e.dark_patch <= 1;
        e.guided = plan_guided(s, r);
        // Strategies 1 and 2 and the dict surface never store the restored image: the histogram sweep (which also files the
        // elements of the predicted target bins, select_lin_begin), the collecting sweep and the stretch each recompute it from
        // the frame and t (restore.h: 11 + 14 bytes per pixel instead of 23 + 15 in float32, and no collecting sweep; the
        // float64 image would be 24 B/px); so do the key-digit passes of planes the selection flags and -- round 4 -- the
        // selection's fallback.  Tuning restore_store keeps the stored planes (4K x 64: 17.9 vs 17.5 ms per step, round 2);
        // the tests compare both modes.  Strategy 3's tail reads the planes and the key sweeps (select_generic) work on them.
        const bool tail_reads_planes = six && p->strategy == 3;
        e.store = e.generic || tu.restore_store || tail_reads_planes;
        // The float32 planes (12 B/px) exist only where they are stored: a 4K x 64 strategy-2 call went 43 -> 31 B/px; the
        // code-domain strategies never had a use for them.  The dict surface's float64 planes keep their place in the layout
        // even when nothing is written to them: the sizes uwie_workspace_bytes answers are pinned.
        e.F = six && e.store;
        e.F64 = p->surface == UWIE_SURFACE_DICT;
        // Strategy 3 keeps the planes, so the exact target bins can be collected from them by one streaming sweep: no predicted
        // windows there -- its percentiles (20 / 85 / 2 / 98) sit where the bins are full and four windows made the restore
        // sweep 2.9 ms at 4K x 16 against 0.65 + 0.35 for sweep + collection.  Tuning lin_predict3 brings the windows back.
        e.predict = !tail_reads_planes || tu.lin_predict3;
        // round 4: no histogram at all -- counts below the predicted windows + the windows' members (k_restore_rank).
        // (small jobs keep the histogram sweep: at 1080p x 1 the rank-counting kernels' fixed costs -- wavefront-private queues,
        // a window-wide list for the finish -- make them 54 + 20 us against 34 + 14; tuning rank_sweep = 2 forces them anyway)
        const bool big = (size_t)s.B * s.npx() >= ((size_t)1 << 24) || tu.rank_sweep >= 2;
        e.rank = six && !e.store && !e.guided.t_f32 && tu.rank_sweep && big && s.npx() >= 4;
        // round 4: cast detection's chunk pass leaves the level-0 quadrant histograms of the quadtree behind (six_stadigy surface
        // with cast detection on; frames entry_fuse_takes)
        e.qpart = six && p->cast_correct && p->forced_cast < 0 && entry_fuse_takes(s, p->min_size);
        e.cast_gray = e.qpart && tu.entry_fuse != 2;
    }
    size_scratch(e, s);
    return e;
}

// The layout that holds every one of the six six_stadigy sets of uwie_enhance_all_u8, which runs them from one workspace: the
// union of their plans (the stored planes if any set keeps them, the exact-order filter's planes if any dehazing set's plan
// needs them, the largest CLAHE tile grid).  six[k]: each set's own plan, which its tail runs in this layout.
EnhancePlan plan_enhance_all(Shape s, const uwie_params *p6, EnhancePlan *six)
{
    EnhancePlan u{};
    u.pipeline = EP_SIX_DEHAZE;
    u.dehaze = true;
    for (int k = 0; k < 6; ++k) {
        const EnhancePlan &e = six[k] = plan_enhance(s, &p6[k]);
        u.F |= e.F;
        u.guided.planes |= e.guided.planes;
        u.qpart |= e.qpart;
        u.tx = std::max(u.tx, e.tx);
        u.ty = std::max(u.ty, e.ty);
    }
    size_scratch(u, s);
    return u;
}

Pipe carve_pipe(Carver &c, Shape s, const EnhancePlan &e)
{
    Pipe P{};
    const size_t n = (size_t)s.B * s.npx();
    P.kind = c.take<int32_t>(s.B);
    P.A = c.take<float>((size_t)s.B * 3);
    P.pct = c.take<float>((size_t)s.B * 3 * kMaxPct);
    P.guess = c.take<int32_t>(s.B);
    if (e.F64) {
        P.F64 = c.take<double>(n * 3);
        P.pct64 = c.take<double>((size_t)s.B * 3 * kMaxPct);
    }
    if (e.F) P.F = c.take<float>(n * 3);
    if (e.dehaze) {
        P.gray = c.take<uint8_t>(n);
        if (!e.t0_in_scratch) P.t0 = c.take<float>(n);
        P.t = c.take<double>(n);
    }
    P.scratch_bytes = e.scratch_bytes;
    P.scratch = c.take<char>(P.scratch_bytes);
    P.planes = e.guided.planes;
    if (e.t0_in_scratch) P.t0 = static_cast<float *>(P.scratch);
    if (e.qpart && P.scratch) P.qpart = reinterpret_cast<uint32_t *>(static_cast<char *>(P.scratch) + e.qoff);
    return P;
}

// The guided filter of a u8 dehazing call on P's buffers: t0 from `frame` (k_trans_init / k_trans_patch into P.t0, or inside
// the fused kernel), then t (float32 data for t_f32 plans; everything downstream reads it through RestoreSrc::t32).
int stage_guided(const Pipe &P, Shape s, const EnhancePlan &e, const FuseT0Args &frame, hipStream_t st)
{
    const GuidedPlan &g = e.guided;
    // the exact-order filter builds its planes in the scratch, where t0 lives otherwise (enhance_all runs each set's own plan
    // in one merged layout)
    UWIE_REQUIRE(!g.planes || (P.planes && P.t0 != P.scratch), "guided filter: the workspace layout has no planes for the exact-order filter");
    if (g.t0) UWIE_TRY(launch_t0(frame, e.dark_patch, s, P.t0, st));
    return launch_guided_plan(g, s, P.gray, P.t0, P.t, P.scratch, st, &frame);
}

// enhance_contrast / white_balance (S6:191-199 / :211-219) of a float32 HWC image: two percentiles into pct [B][3][2], then
// the stretch to `out` (which may be img)
int stretch_f32(const float *img, float *out, Shape s, double lo, double hi, float eps, float *pct, void *ws, hipStream_t st)
{
    const double q[2] = {lo, hi};
    UWIE_TRY(launch_percentiles(img, 0, s, q, 2, pct, ws, st));
    return launch_stretch_apply_f32(img, pct, 2, 0, 1, eps, out, s, st);
}

// Cast detection (or the forced kind): what every six_stadigy strategy starts from.
int six_cast(uwie_ctx *ctx, const uint8_t *d_in, Shape s, const EnhancePlan &e, const uwie_params *p, const Pipe &P,
             const int32_t **kind, hipStream_t st)
{
    *kind = nullptr;
    if (p->forced_cast >= 0) {
        UWIE_TRY(launch_set_kind(P.kind, s.B, p->forced_cast, st));
        *kind = P.kind;
    } else if (p->cast_correct) {
        const EntryFuse ef{P.qpart, e.cast_gray ? P.gray : nullptr, P.guess, p->gray_shift};
        UWIE_TRY(launch_cast_classify(ctx, d_in, s, P.kind, nullptr, P.scratch, st, e.qpart ? &ef : nullptr));
        *kind = P.kind;
    }
    return UWIE_OK;
}

// Gray plane and atmospheric light: they depend on the (colour-corrected) frame only, so strategies 1-3 share them.
int six_airlight(uwie_ctx *ctx, const uint8_t *d_in, const int32_t *kind, Shape s, const EnhancePlan &e, const uwie_params *p,
                 const Pipe &P, hipStream_t st)
{
    // (gray_shift 0: the plane is there already -- cast detection's chunk pass wrote it)
    return launch_airlight(ctx, d_in, kind, P.gray, s, p->min_size, P.A, nullptr, P.scratch, st, e.cast_gray ? 0 : p->gray_shift,
                           e.qpart ? P.qpart : nullptr);
}

// Strategies 1-3 from (kind, gray, A) on: transmission -> guided filter -> restore -> stretch -> CLAHE / white balance.
int six_dehaze_tail(uwie_ctx *ctx, const uint8_t *d_in, const int32_t *kind, Shape s, const EnhancePlan &e, const uwie_params *p,
                    const Pipe &P, uint8_t *d_out_u8, float *d_out_f32, hipStream_t st)
{
    const float eps = 1e-6f;  // six_stadigy.py:198,218
    const int k = p->strategy, nq = k == 3 ? 4 : 2, t_is_f32 = e.guided.t_f32;
    UWIE_TRY(stage_guided(P, s, e, FuseT0Args{d_in, kind, P.A, (float)p->omega, 1e-6f, 1}, st));  // S6:170-180
    // fused tail: restore feeds the selection's first histogram sweep (and writes the planar image into P.F where it is stored)
    SelectPlan plan;
    const double q[4] = {p->L_low, p->L_high, p->wb_percentile, 100 - p->wb_percentile};
    const RestoreSrc src{d_in, kind, P.A, P.t, t_is_f32};
    const RestoreSrc *recompute = e.store ? nullptr : &src;
    if (e.generic) {
        UWIE_TRY(select_begin<float>(s, q, nq, P.scratch, st, &plan));
        UWIE_TRY(launch_restore_planar_hist(d_in, kind, P.A, P.t, s, P.F, plan.ghist, st, false, nullptr, t_is_f32));
        UWIE_TRY(select_run(plan, P.F, 1, s, true, st));
    } else {
        // the restored image is clipped to [0, 1]: linear first digit, one collecting sweep (k_select.hip, select_lin_*)
        UWIE_TRY(select_lin_begin<float>(s, q, nq, P.scratch, st, &plan, e.predict ? &src : nullptr));
        if (e.rank && plan.predicted) {
            UWIE_TRY(launch_restore_rank(src, s, plan, st));
            UWIE_TRY(select_rank_run(plan, s, st, src));
        } else {
            UWIE_TRY(launch_restore_planar_hist(d_in, kind, P.A, P.t, s, e.store ? P.F : nullptr, plan.ghist, st, true, &plan, t_is_f32));
            UWIE_TRY(select_lin_run(plan, P.F, s, st, recompute));
        }
    }
    if (k == 3) {
        UWIE_TRY(select_lerp_chain(plan, s, eps, P.pct, st));
        return launch_tail_plain(P.F, P.pct, 4, eps, 1, s, 0, 1.0, d_out_u8, d_out_f32, st);
    }
    UWIE_TRY(select_lerp(plan, s, P.pct, st));
    return launch_tail_clahe(ctx, P.F, P.pct, 2, eps, 0, s, p->clip_limit, e.tx, e.ty, k == 1 ? 1 : 0, p->gamma, d_out_u8, d_out_f32,
                             P.scratch, st, recompute);
}

// enhancement_strategies.py apply_strong/medium/light (ES:350-444) on the uncorrected frame
// have_airlight: P.gray and P.A already hold the gray plane and the atmospheric light of these frames (they depend on the
// frame, min_size and gray_shift only: ES:353,379,425 all call estimate_atmospheric_light(img) -- uwie_select_best_u8 shares them)
int dict_dehaze(uwie_ctx *ctx, const uint8_t *d_in, Shape s, const EnhancePlan &e, const uwie_params *p, const Pipe &P,
                uint8_t *d_out_u8, float *d_out_f32, double *d_out_f64, hipStream_t st, bool have_airlight)
{
    if (!have_airlight)
        UWIE_TRY(launch_airlight(ctx, d_in, nullptr, P.gray, s, p->min_size, P.A, nullptr, P.scratch, st, p->gray_shift));
    UWIE_TRY(stage_guided(P, s, e, FuseT0Args{d_in, nullptr, P.A, (float)p->omega, 1e-10f, 0}, st));  // ES:221-232
    SelectPlan plan;
    const double q[2] = {p->L_low, p->L_high};
    const RestoreSrc src{d_in, nullptr, P.A, P.t};
    const RestoreSrc *recompute = e.store ? nullptr : &src;
    if (e.generic) {
        UWIE_TRY(select_begin<double>(s, q, 2, P.scratch, st, &plan));
        UWIE_TRY(launch_recover64_planar_hist(d_in, P.A, P.t, s, P.F64, plan.ghist, st));
        UWIE_TRY(select_run(plan, P.F64, 1, s, true, st));
    } else {
        // the recovered image is clipped to [0, 1]: linear first digit, one collecting sweep (select_lin_*<double>)
        UWIE_TRY(select_lin_begin<double>(s, q, 2, P.scratch, st, &plan, &src));
        UWIE_TRY(launch_recover64_planar_hist(d_in, P.A, P.t, s, e.store ? P.F64 : nullptr, plan.ghist, st, true, &plan));
        UWIE_TRY(select_lin_run(plan, P.F64, s, st, recompute));
    }
    UWIE_TRY(select_lerp(plan, s, P.pct64, st));
    return launch_tail_plain64(P.F64, P.pct64, s, p->apply_gamma, p->gamma, d_out_u8, d_out_f32, st, recompute, d_out_f64);
}

// Runs a u8 call as planned on P's buffers: the strategy's float image goes to d_out_f32 / d_out_f64 (dict surface) and / or
// its (y*255).astype(u8) image to d_out_u8.  have_airlight: see dict_dehaze.
int run_enhance(uwie_ctx *ctx, const uint8_t *d_in, Shape s, const EnhancePlan &e, const uwie_params *p, const Pipe &P,
                uint8_t *d_out_u8, float *d_out_f32, double *d_out_f64, hipStream_t st, bool have_airlight = false)
{
    const int32_t *kind = nullptr;
    switch (e.pipeline) {
    case EP_SIX_DEHAZE:
        UWIE_TRY(six_cast(ctx, d_in, s, e, p, P, &kind, st));
        UWIE_TRY(six_airlight(ctx, d_in, kind, s, e, p, P, st));
        return six_dehaze_tail(ctx, d_in, kind, s, e, p, P, d_out_u8, d_out_f32, st);
    case EP_SIX_CODES:  // strategies 4-6 never leave 8-bit data for long: evaluated as per-image LUT chains (k_codes.hip)
        UWIE_TRY(six_cast(ctx, d_in, s, e, p, P, &kind, st));
        return launch_code_strategy(ctx, d_in, kind, s, p, d_out_u8, d_out_f32, P.scratch, st);
    case EP_DICT_DEHAZE: return dict_dehaze(ctx, d_in, s, e, p, P, d_out_u8, d_out_f32, d_out_f64, st, have_airlight);
    default: return launch_code_strategy(ctx, d_in, nullptr, s, p, d_out_u8, d_out_f32, P.scratch, st, d_out_f64);
    }
}

int check_params(const uwie_params *p)
{
    UWIE_REQUIRE(p != nullptr, "params is NULL");
    UWIE_REQUIRE(p->surface == UWIE_SURFACE_SIX || p->surface == UWIE_SURFACE_DICT, "unknown surface");
    if (p->surface == UWIE_SURFACE_SIX) UWIE_REQUIRE(p->strategy >= 1 && p->strategy <= 6, "unknown strategy");
    else UWIE_REQUIRE(p->strategy >= 0 && p->strategy <= 4, "unknown strategy");
    UWIE_REQUIRE(p->gray_shift == 14 || p->gray_shift == 15, "gray_shift must be 14 or 15");
    UWIE_REQUIRE(p->forced_cast >= -1 && p->forced_cast <= 2, "forced_cast must be -1 or a UWIE_CAST_* kind");
    UWIE_REQUIRE(p->min_size >= 1, "min_size must be >= 1");
    UWIE_REQUIRE(p->tiles_x >= 1 && p->tiles_y >= 1 && p->tiles_x * p->tiles_y <= 4096, "bad CLAHE tile grid");
    if (dehazes(p)) UWIE_REQUIRE(p->gf_ksize >= 1 && p->gf_ksize <= 1024, "guided-filter width out of range");
    // np.percentile raises ValueError("Percentiles must be in the range [0, 100]") for these (also for NaN)
    UWIE_REQUIRE(p->L_low >= 0.0 && p->L_low <= 100.0 && p->L_high >= 0.0 && p->L_high <= 100.0,
                 "L_low / L_high must be percentiles in [0, 100]");
    if (p->surface == UWIE_SURFACE_SIX && (p->strategy >= 3 && p->strategy <= 5))
        UWIE_REQUIRE(p->wb_percentile >= 0.0 && p->wb_percentile <= 100.0, "wb_percentile must be in [0, 100]");
    UWIE_REQUIRE(p->inter_dtype == UWIE_INTER_F64 || p->inter_dtype == UWIE_INTER_FX32 || p->inter_dtype == UWIE_INTER_F32T,
                 "unknown inter_dtype");
    UWIE_REQUIRE(p->dark_patch >= 0 && p->dark_patch <= 31, "dark_patch must be 0 .. 31 (0 and 1: the per-pixel dark channel)");
    return UWIE_OK;
}


// ---------------------------------------------------------------- general float images (k_float.hip)
// Buffers of one float-image call.  T = the image's dtype (float: either surface; double: dict surface only).
template <class T>
struct FloatPipe {
    int32_t *kind;
    T *A;
    float *pct;
    double *pct64;
    T *xc;          // colour-corrected copy (SIX surface with cast correction)
    uint8_t *q;     // (x * 255).astype(u8)
    uint8_t *gray;
    T *t0;
    double *t;
    float *F, *F2;  // SIX: working images, HWC
    double *F64;    // DICT: recovered image, planar
    void *scratch;
    size_t scratch_bytes;
};

template <class T>
FloatPipe<T> carve_float(Carver &c, Shape s, const uwie_params *p)
{
    FloatPipe<T> P{};
    const size_t n = (size_t)s.B * s.npx();
    const bool six = p->surface == UWIE_SURFACE_SIX, dz = dehazes(p);
    P.kind = c.take<int32_t>(s.B);
    P.A = c.take<T>((size_t)s.B * 3);
    P.pct = c.take<float>((size_t)s.B * 3 * kMaxPct);
    P.pct64 = c.take<double>((size_t)s.B * 3 * kMaxPct);
    if (six) P.xc = c.take<T>(n * 3);
    P.q = c.take<uint8_t>(n * 3);
    if (dz) {
        P.gray = c.take<uint8_t>(n);
        P.t0 = c.take<T>(n);
        P.t = c.take<double>(n);
    }
    if (six) {
        P.F = c.take<float>(n * 3);
        P.F2 = c.take<float>(n * 3);
    } else if (dz) {
        P.F64 = c.take<double>(n * 3);
    }
    const int tx = p->tiles_x > 0 ? p->tiles_x : 8, ty = p->tiles_y > 0 ? p->tiles_y : 8;
    const size_t none = 0;
    P.scratch_bytes = std::max({dz ? float_airlight_ws_bytes(s) : none, dz ? guided_ws_bytes(s) : none, select_ws_bytes(s),
                                clahe_ws_bytes(s, tx, ty), codes_ws_bytes(s, tx, ty)});
    P.scratch = c.take<char>(P.scratch_bytes);
    return P;
}

// percentile stretch of a float32 HWC image in place (S6:191-199 / :211-219)
static int float_stretch(const FloatPipe<float> &P, float *img, Shape s, double lo, double hi, hipStream_t st)
{
    return stretch_f32(img, img, s, lo, hi, 1e-6f, P.pct, P.scratch, st);
}

// six_stadigy.py strategies 1-6 on a float32 image (S6:230-285); the result image goes to out_f32 and/or out_u8
static int run_float_six(uwie_ctx *ctx, const float *d_img, Shape s, const uwie_params *p, const FloatPipe<float> &P, uint8_t *out_u8,
                         float *out_f32, hipStream_t st)
{
    const size_t n3 = (size_t)s.B * s.npx() * 3;
    const int32_t *kind = nullptr;
    if (p->forced_cast >= 0) {
        UWIE_TRY(launch_set_kind(P.kind, s.B, p->forced_cast, st));
        kind = P.kind;
    } else if (p->cast_correct) {
        UWIE_TRY(launch_float_cast_classify<float>(d_img, s, P.kind, nullptr, st));
        kind = P.kind;
    }
    const int k = p->strategy;
    const bool dz = k <= 3;
    const float *x = d_img;
    UWIE_TRY(launch_float_prepare<float>(d_img, kind, kind ? P.xc : nullptr, dz ? P.q : nullptr, s, st));
    if (kind) x = P.xc;
    float *y = P.F;
    if (dz) {
        UWIE_TRY(launch_rgb2gray_u8(P.q, P.gray, (size_t)s.B * s.npx(), p->gray_shift, st));
        UWIE_TRY(launch_float_airlight<float>(x, P.gray, s, p->min_size, P.A, P.scratch, st));
        UWIE_TRY(launch_float_trans_init<float>(x, P.A, s, p->omega, (double)1e-6f, 1, P.t0, st));
        UWIE_TRY(launch_guided_plan(plan_guided(s, {p->gf_ksize, p->gf_eps, p->gf_exact != 0}), s, P.gray, P.t0, P.t, P.scratch, st));
        UWIE_TRY((launch_float_restore<float, float>(x, P.A, P.t, s, y, 0, st)));
        UWIE_TRY(float_stretch(P, y, s, p->L_low, p->L_high, st));
        if (k == 3) {
            UWIE_TRY(float_stretch(P, y, s, p->wb_percentile, 100 - p->wb_percentile, st));
        } else {
            UWIE_TRY(launch_clahe_f32(ctx, y, P.F2, s, p->clip_limit, p->tiles_x, p->tiles_y, P.scratch, st));
            y = P.F2;
            if (k == 1) UWIE_TRY(launch_gamma_f32(y, y, n3, p->gamma, 1, st));
        }
    } else if (k == 4) {  // S6:262-268  clahe -> stretch -> white_balance -> gamma
        UWIE_TRY(launch_clahe_f32(ctx, x, y, s, p->clip_limit, p->tiles_x, p->tiles_y, P.scratch, st));
        UWIE_TRY(float_stretch(P, y, s, p->L_low, p->L_high, st));
        UWIE_TRY(float_stretch(P, y, s, p->wb_percentile, 100 - p->wb_percentile, st));
        UWIE_TRY(launch_gamma_f32(y, y, n3, p->gamma, 1, st));
    } else {  // S6:270-285  [white_balance ->] stretch -> clahe -> gamma
        UWIE_HIP_CHECK(hipMemcpyAsync(y, x, n3 * sizeof(float), hipMemcpyDeviceToDevice, st));
        if (k == 5) UWIE_TRY(float_stretch(P, y, s, p->wb_percentile, 100 - p->wb_percentile, st));
        UWIE_TRY(float_stretch(P, y, s, p->L_low, p->L_high, st));
        UWIE_TRY(launch_clahe_f32(ctx, y, P.F2, s, p->clip_limit, p->tiles_x, p->tiles_y, P.scratch, st));
        y = P.F2;
        UWIE_TRY(launch_gamma_f32(y, y, n3, p->gamma, 1, st));
    }
    if (out_f32) UWIE_HIP_CHECK(hipMemcpyAsync(out_f32, y, n3 * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (out_u8) UWIE_TRY(launch_quantise_u8(y, out_u8, n3, st));
    return UWIE_OK;
}

// enhancement_strategies.py apply_strategy bodies (ES:350-474) on a float32 or float64 image
template <class T>
static int run_float_dict(uwie_ctx *ctx, const T *d_img, Shape s, const uwie_params *p, const FloatPipe<T> &P, uint8_t *out_u8,
                          float *out_f32, double *out_f64, hipStream_t st)
{
    UWIE_TRY(launch_float_prepare<T>(d_img, nullptr, (T *)nullptr, P.q, s, st));
    if (!dehazes(p))  // clahe_enhancement / histogram_equalization start by quantising: code domain from here on
        return launch_code_strategy(ctx, P.q, nullptr, s, p, out_u8, out_f32, P.scratch, st, out_f64, true);
    UWIE_TRY(launch_rgb2gray_u8(P.q, P.gray, (size_t)s.B * s.npx(), p->gray_shift, st));
    UWIE_TRY(launch_float_airlight<T>(d_img, P.gray, s, p->min_size, P.A, P.scratch, st));
    UWIE_TRY(launch_float_trans_init<T>(d_img, P.A, s, p->omega, 1e-10, 0, P.t0, st));  // ES:221-225: no clip
    GuidedRequest r{p->gf_ksize, p->gf_eps, p->gf_exact != 0};
    r.t0_f64 = sizeof(T) == 8;  // float64 images: the exact-order kernels
    UWIE_TRY(launch_guided_plan(plan_guided(s, r), s, P.gray, P.t0, P.t, P.scratch, st));
    UWIE_TRY((launch_float_restore<T, double>(d_img, P.A, P.t, s, P.F64, 1, st)));
    SelectPlan plan;
    const double q[2] = {p->L_low, p->L_high};
    UWIE_TRY(select_begin<double>(s, q, 2, P.scratch, st, &plan));
    UWIE_TRY(select_run(plan, P.F64, 1, s, false, st));
    UWIE_TRY(select_lerp(plan, s, P.pct64, st));
    return launch_tail_plain64(P.F64, P.pct64, s, p->apply_gamma, p->gamma, out_u8, out_f32, st, nullptr, out_f64);
}

template <class T>
static size_t float_ws_bytes(int batch, int H, int W, const uwie_params *p)
{
    Carver c(nullptr);
    carve_float<T>(c, Shape{batch, H, W}, p);
    return c.total();
}

// ---------------------------------------------------------------- the learned stack's handles
// A handle's device made current for a scope and the previous one put back; nothing when it is current already or the
// query fails.  (The handle's functions that take no context: *_destroy, uwie_mlp_trainer_get / _set.)
class DeviceGuard {
public:
    explicit DeviceGuard(int device)
        : switched_(hipGetDevice(&prev_) == hipSuccess && prev_ != device && hipSetDevice(device) == hipSuccess)
    {
    }
    ~DeviceGuard()
    {
        if (switched_) (void)hipSetDevice(prev_);
    }
    DeviceGuard(const DeviceGuard &) = delete;

private:
    int prev_ = -1;  // declared (so initialised) before switched_
    bool switched_;
};

// uwie_vgg, uwie_param_net, uwie_mlp and uwie_model: a network of device pointers into one allocation on `device`
template <class Net>
struct Handle {
    int device;
    Net net;
    void *blob;
};

template <class H>
void handle_destroy(H *h)
{
    if (!h) return;
    DeviceGuard on(h->device);
    (void)hipFree(h->blob);
    delete h;
}

// The end of every *_create (who): rc of the pack on the null stream, then its completion.  On either failure `cleanup`
// runs, and a HIP error becomes the message.
template <class F>
int pack_finish(int rc, const char *who, F cleanup, const char *what = "packing failed: ")
{
    const hipError_t e = rc == UWIE_OK ? hipStreamSynchronize(nullptr) : hipSuccess;
    if (rc == UWIE_OK && e == hipSuccess) return UWIE_OK;
    cleanup();
    if (e != hipSuccess) set_error("%s: %s%s", who, what, hipGetErrorString(e));
    return rc != UWIE_OK ? rc : UWIE_E_HIP;
}

#define UWIE_REQUIRE_F(cond, ...)       \
    do {                                \
        if (!(cond)) {                  \
            set_error(__VA_ARGS__);     \
            return UWIE_E_INVALID;      \
        }                               \
    } while (0)

// What the entry points that take rows of an MLP share, in their order: NULL pointers, the device of the handle (a
// uwie_mlp, "the network", or a uwie_mlp_trainer), the batch (an eval forward takes more rows than a training step keeps
// activations for), the alignment of the rows and of the float32 array `d_other` that goes with them.
constexpr int kMlpEvalBatch = 1 << 20, kMlpTrainBatch = 65536;
template <class H>
int mlp_rows_check(const char *who, const uwie_ctx *ctx, const H *h, const void *d_features, int features_are_f64, int batch,
                   bool training, const float *d_other, const char *other_name)
{
    UWIE_REQUIRE_F(ctx && h && d_features && d_other, "%s: NULL pointer", who);
    UWIE_REQUIRE_F(h->device == ctx->device, "%s: the %s lives on another device", who,
                   std::is_same<H, uwie_mlp>::value ? "network" : "trainer");
    UWIE_REQUIRE_F(batch >= 1 && batch <= (training ? kMlpTrainBatch : kMlpEvalBatch), "%s: batch out of range (1 .. %s)", who,
                   training ? "65536" : "2^20");
    UWIE_REQUIRE_F(((uintptr_t)d_features & (features_are_f64 ? 7 : 3)) == 0 && ((uintptr_t)d_other & 3) == 0,
                   "%s: d_features and %s must be aligned for their element types", who, other_name);
    return UWIE_OK;
}

// The flags of an enhancement module (map: UWIE_LOSS_VGG, or UWIE_LOSS_GATED whose flags are reserved) and what the entry
// point `who` says about bad ones; ReferenceLoss, which takes either module, names it as well.
bool module_flags_ok(int map, int flags) { return map == UWIE_LOSS_VGG ? (flags & ~3) == 0 : flags == 0; }
int module_flags_check(const char *who, int map, int flags, bool name_module = false)
{
    const bool vgg = map == UWIE_LOSS_VGG;
    UWIE_REQUIRE_F(module_flags_ok(map, flags), "%s: %sflags are %s", who, !name_module ? "" : vgg ? "vgg " : "gated ",
                   vgg ? "UWIE_DIFF_OMEGA | UWIE_DIFF_GAMMA" : "reserved (0)");
    return UWIE_OK;
}

}  // namespace
}  // namespace uwie

using namespace uwie;

extern "C" {

const char *uwie_last_error(void) { return g_err; }
const char *uwie_version(void) { return "uwie 0.1 (gfx950)"; }

int uwie_create(int device, uwie_ctx **out_ctx)
{
    UWIE_REQUIRE(out_ctx != nullptr, "out_ctx is NULL");
    *out_ctx = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        set_error("no HIP device available (libuwie has no CPU path)");
        return UWIE_E_NODEVICE;
    }
    UWIE_REQUIRE(device >= 0 && device < count, "device index out of range");
    UWIE_HIP_CHECK(hipSetDevice(device));
    int cus = 0;
    UWIE_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    uwie_ctx *ctx = new uwie_ctx();
    ctx->aux_ready = false;
    ctx->prof = prof_create();
    ctx->device = device;
    ctx->cus = cus;
    tuning_from_env(&ctx->tune);
    LabTables *lab = new LabTables();
    CastTables *cast = new CastTables();
    build_lab_tables(lab);
    build_cast_tables(cast);
    hipError_t e = hipMalloc((void **)&ctx->d_lab, sizeof(LabTables));
    if (e == hipSuccess) e = hipMalloc((void **)&ctx->d_cast, sizeof(CastTables));
    if (e == hipSuccess) e = hipMalloc((void **)&ctx->d_status, 64);
    if (e == hipSuccess) e = hipMemset(ctx->d_status, 0, 64);
    if (e == hipSuccess) e = hipMemcpy(ctx->d_lab, lab, sizeof(LabTables), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(ctx->d_cast, cast, sizeof(CastTables), hipMemcpyHostToDevice);
    delete lab;
    delete cast;
    if (e != hipSuccess) {
        set_error("context table upload failed: %s", hipGetErrorString(e));
        uwie_destroy(ctx);
        return UWIE_E_HIP;
    }
    *out_ctx = ctx;
    return UWIE_OK;
}

void uwie_destroy(uwie_ctx *ctx)
{
    if (!ctx) return;
    if (ctx->d_lab) (void)hipFree(ctx->d_lab);
    if (ctx->d_cast) (void)hipFree(ctx->d_cast);
    if (ctx->d_status) (void)hipFree(ctx->d_status);
    if (ctx->aux_ready) {
        for (int i = 0; i < 4; ++i) {
            (void)hipStreamDestroy(ctx->aux[i]);
            (void)hipEventDestroy(ctx->join[i]);
        }
        (void)hipEventDestroy(ctx->fork);
    }
    prof_bind(nullptr);
    prof_destroy(ctx->prof);
    delete ctx;
}

int uwie_device_status(uwie_ctx *ctx, void *stream, uint32_t *bits)
{
    UWIE_REQUIRE(ctx != nullptr, "device_status: NULL context");
    UWIE_SCOPE(ctx);
    uint32_t v = 0;
    hipStream_t st = (hipStream_t)stream;
    UWIE_HIP_CHECK(hipMemcpyAsync(&v, ctx->d_status, sizeof v, hipMemcpyDeviceToHost, st));
    UWIE_HIP_CHECK(hipStreamSynchronize(st));
    if (v) UWIE_HIP_CHECK(hipMemsetAsync(ctx->d_status, 0, sizeof v, st));
    if (bits) *bits = v;
    if (v) {
        set_error("device status 0x%x:%s the results of the calls since the last check are not valid", v,
                  (v & UWIE_STATUS_CANNY_LABEL) ? " Canny hysteresis met a component label that this launch did not write (k_canny.hip);"
                  : (v & UWIE_STATUS_QTREE_BOUNDS) ? " a quadtree score fell outside its histogram interval (k_airlight.hip, tuning q_hist = 3);"
                  : (v & UWIE_STATUS_FEATURE_COUNTS) ? " a frame's feature histograms do not count every pixel (k_extractor.hip);"
                  : (v & UWIE_STATUS_DIFF_RANK) ? " a gated DifferentiableEnhancement image has no valid sorted position (an IndexError, ValueError or OverflowError in Python);"
                  : (v & UWIE_STATUS_RESIZE_DESC) ? " a resize frame descriptor has a NULL pointer or a size out of range (k_resize.hip);"
                  : (v & UWIE_STATUS_CLASSIFY_NAN) ? " a row holds NaN and the model is GB or SVC (scikit-learn: ValueError, Input X contains NaN);" : "");
        return UWIE_E_DEVICE;
    }
    return UWIE_OK;
}

int uwie_device_status_async(uwie_ctx *ctx, uint32_t *d_bits, void *stream)
{
    UWIE_REQUIRE(ctx && d_bits, "device_status_async: NULL pointer");
    UWIE_SCOPE(ctx);
    hipStream_t st = (hipStream_t)stream;
    UWIE_HIP_CHECK(hipMemcpyAsync(d_bits, ctx->d_status, sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    UWIE_HIP_CHECK(hipMemsetAsync(ctx->d_status, 0, sizeof(uint32_t), st));
    return UWIE_OK;
}

int uwie_profile_enable(uwie_ctx *ctx, int on)
{
    UWIE_REQUIRE(ctx != nullptr, "profile_enable: NULL context");
    prof_enable(ctx->prof, on != 0);
    prof_bind(on ? ctx->prof : nullptr);
    return UWIE_OK;
}

int uwie_profile_filter(uwie_ctx *ctx, const char *kernel_name)
{
    UWIE_REQUIRE(ctx != nullptr, "ctx is NULL");
    prof_filter(ctx->prof, kernel_name);
    return UWIE_OK;
}

int uwie_profile_collect(uwie_ctx *ctx)
{
    if (!ctx) {
        set_error("profile_collect: NULL context");
        return UWIE_E_INVALID;
    }
    return prof_collect(ctx->prof);
}

int uwie_profile_row(uwie_ctx *ctx, int i, const char **name, double *total_ms, int *calls)
{
    UWIE_REQUIRE(ctx && name && total_ms && calls, "profile_row: NULL pointer");
    return prof_row(ctx->prof, i, name, total_ms, calls);
}

int uwie_set_tuning(uwie_ctx *ctx, const char *name, int value)
{
    UWIE_REQUIRE(ctx && name, "set_tuning: NULL pointer");
    for (const KnobName &k : kKnobs)
        if (std::strcmp(k.name, name) == 0) {
            ctx->tune.*(k.field) = value;
            return UWIE_OK;
        }
    set_error("set_tuning: unknown selector '%s'", name);
    return UWIE_E_INVALID;
}

int uwie_get_tuning(uwie_ctx *ctx, const char *name, int *value)
{
    UWIE_REQUIRE(ctx && name && value, "get_tuning: NULL pointer");
    for (const KnobName &k : kKnobs)
        if (std::strcmp(k.name, name) == 0) {
            *value = ctx->tune.*(k.field);
            return UWIE_OK;
        }
    set_error("get_tuning: unknown selector '%s'", name);
    return UWIE_E_INVALID;
}

int uwie_params_init(uwie_params *p, int surface, int strategy)
{
    UWIE_REQUIRE(p != nullptr, "params is NULL");
    std::memset(p, 0, sizeof *p);
    p->surface = surface;
    p->strategy = strategy;
    p->gray_shift = 15;
    p->min_size = 1;
    p->tiles_x = p->tiles_y = 8;
    p->wb_percentile = -1.0;
    p->gamma = 1.2;
    p->forced_cast = -1;
    p->dark_patch = 1;
    if (surface == UWIE_SURFACE_SIX) {
        p->cast_correct = 1;
        switch (strategy) {  // six_stadigy.py:230-285
        case 1: p->omega = 0.3; p->gf_ksize = 20; p->gf_eps = 5e-1; p->L_low = 5; p->L_high = 98; p->clip_limit = 3.0; p->gamma = 1.5; p->apply_gamma = 1; break;
        case 2: p->omega = 0.5; p->gf_ksize = 15; p->gf_eps = 5e-1; p->L_low = 15; p->L_high = 95; p->clip_limit = 2.0; break;
        case 3: p->omega = 0.7; p->gf_ksize = 10; p->gf_eps = 1e-1; p->L_low = 20; p->L_high = 85; p->wb_percentile = 2; break;
        case 4: p->clip_limit = 4.0; p->L_low = 10; p->L_high = 95; p->wb_percentile = 3; p->gamma = 1.3; p->apply_gamma = 1; break;
        case 5: p->wb_percentile = 2; p->L_low = 15; p->L_high = 90; p->clip_limit = 1.5; p->gamma = 1.2; p->apply_gamma = 1; break;
        case 6: p->L_low = 5; p->L_high = 98; p->clip_limit = 3.5; p->gamma = 1.4; p->apply_gamma = 1; break;
        default: set_error("unknown strategy %d", strategy); return UWIE_E_INVALID;
        }
        return UWIE_OK;
    }
    if (surface == UWIE_SURFACE_DICT) {
        p->gf_eps = 0.001;  // estimate_transmission's default; callers never pass it (ES:209,354-358)
        switch (strategy) {  // in-code defaults of ES:350-474
        case UWIE_DICT_STRONG_DEHAZING: p->omega = 0.5; p->gf_ksize = 15; p->L_low = 10; p->L_high = 95; break;
        case UWIE_DICT_MEDIUM_DEHAZING: p->omega = 0.6; p->gf_ksize = 20; p->L_low = 15; p->L_high = 92; break;
        case UWIE_DICT_LIGHT_ENHANCEMENT: p->omega = 0.4; p->gf_ksize = 10; p->L_low = 15; p->L_high = 95; break;
        case UWIE_DICT_CLAHE_ENHANCEMENT: p->clip_limit = 2.0; p->L_low = 20; p->L_high = 85; break;
        case UWIE_DICT_HISTOGRAM_EQUALIZATION: p->L_low = 10; p->L_high = 95; break;
        default: set_error("unknown strategy %d", strategy); return UWIE_E_INVALID;
        }
        return UWIE_OK;
    }
    set_error("unknown surface %d", surface);
    return UWIE_E_INVALID;
}

// How many sub-batches uwie_enhance_u8 runs on separate streams: tuning `streams` = 2..4, default 1.
// Two streams shorten a 4K x 64 step by ~3 % because issue-bound and memory-bound stages of different sub-batches overlap;
// it is opt-in because overlapped kernels no longer have a per-kernel duration that means anything (bench.py's roofline
// line and rocprofv3's averages both read 1.8x for the guided filter).
static int enhance_split(int batch)
{
    const int n = std::min(std::max(tune().streams, 1), 4);
    return batch >= n ? n : 1;
}

// The buffers of a uwie_enhance_u8 call that runs its batch as nsplit (1 .. 4, at most the batch) sub-batches: their counts and
// first frames, and for each its own plan and its own slice of the workspace (256-byte aligned; `bytes` is where the last one ends).
struct EnhanceLayout {
    int nsplit;
    int cnt[4], start[4];
    EnhancePlan plan[4];
    Pipe P[4];
    size_t bytes;
};

static EnhanceLayout carve_enhance(void *d_workspace, Shape s, const uwie_params *p, int nsplit)
{
    EnhanceLayout L{};
    L.nsplit = nsplit;
    for (int i = 0, b0 = 0; i < nsplit; b0 += L.cnt[i++]) {
        L.cnt[i] = s.B / nsplit + (i < s.B % nsplit ? 1 : 0);
        L.start[i] = b0;
        const Shape si{L.cnt[i], s.H, s.W};
        Carver c(d_workspace ? static_cast<char *>(d_workspace) + L.bytes : nullptr);
        L.plan[i] = plan_enhance(si, p);
        L.P[i] = carve_pipe(c, si, L.plan[i]);
        L.bytes += c.total();
    }
    return L;
}

// The layout of a call on this workspace: the whole batch in one Pipe, or -- tuning `streams`, may_split -- sub-batches, unless
// the caller's buffer cannot hold their slices (a caller that sized for another parameter set).  uwie_enhance_percentiles finds
// the last call's percentiles by the same carving, so the two cannot disagree.  *need: the single layout's bytes (what the call
// requires of the workspace).
static EnhanceLayout enhance_layout(void *d_workspace, size_t workspace_bytes, Shape s, const uwie_params *p, bool may_split, size_t *need)
{
    const EnhanceLayout whole = carve_enhance(d_workspace, s, p, 1);
    *need = whole.bytes;
    const int nsplit = may_split ? enhance_split(s.B) : 1;
    if (nsplit < 2) return whole;
    const EnhanceLayout split = carve_enhance(d_workspace, s, p, nsplit);
    return split.bytes <= workspace_bytes ? split : whole;
}

size_t uwie_workspace_bytes(int batch, int H, int W, const uwie_params *p)
{
    if (!shape_ok(batch, H, W)) return 0;
    const Shape s{batch, H, W};
    // uwie_enhance_u8 may run the batch as up to four sub-batches on separate streams (tuning `streams`), each with its own
    // slice: sized for whichever split is the largest, so the answer does not depend on a context
    size_t pipe = 0;
    for (int nsplit = 1; nsplit <= 4 && nsplit <= batch; ++nsplit) pipe = std::max(pipe, carve_enhance(nullptr, s, p, nsplit).bytes);
    if (p) return pipe;  // a pipeline call with these parameters
    // p == NULL: any stage entry point; they carve their own (smaller) layouts from the same buffer
    return std::max({pipe, canny_ws_bytes(s) + (size_t)batch * sizeof(Region) + 256, guided_ws_bytes(s), features_ws_bytes(s),
                     quality_ws_bytes(s), clahe_ws_bytes(s, 8, 8), airlight_ws_bytes(s) + (size_t)batch * s.npx() + 256});
}

size_t uwie_workspace_bytes_ctx(uwie_ctx *ctx, int batch, int H, int W, const uwie_params *p)
{
    if (!ctx) return uwie_workspace_bytes(batch, H, W, p);
    CallScope scope(ctx);  // tune() answers for this context
    return uwie_workspace_bytes(batch, H, W, p);
}

size_t uwie_workspace_bytes_all(int batch, int H, int W, const uwie_params *p6)
{
    if (!shape_ok(batch, H, W)) return 0;
    uwie_params P6[6];
    for (int k = 0; k < 6; ++k) {
        if (p6) P6[k] = p6[k];
        else if (uwie_params_init(&P6[k], UWIE_SURFACE_SIX, k + 1) != UWIE_OK) return 0;
    }
    const Shape s{batch, H, W};
    EnhancePlan six[6];
    Carver c(nullptr);
    carve_pipe(c, s, plan_enhance_all(s, P6, six));
    return c.total();
}

int uwie_enhance_u8(uwie_ctx *ctx, const uint8_t *d_in, uint8_t *d_out_u8, float *d_out_f32, int batch, int H, int W,
                    const uwie_params *p, void *d_workspace, size_t workspace_bytes, void *stream)
{
    UWIE_REQUIRE(ctx && d_in && (d_out_u8 || d_out_f32), "enhance: NULL context or image pointer");
    UWIE_SCOPE(ctx);
    UWIE_CHECK_SHAPE(batch, H, W);
    UWIE_TRY(check_params(p));
    size_t need;
    const EnhanceLayout L = enhance_layout(d_workspace, workspace_bytes, Shape{batch, H, W}, p, true, &need);
    UWIE_CHECK_WS(need);
    ctx->last_enhance_f64 = false;
    hipStream_t st = (hipStream_t)stream;
    // Frames are independent, so the batch may run as sub-batches on separate streams: while one sits in an issue-bound
    // stage (guided filter) another can be in a memory-bound one.  The caller's stream waits for all of them.  A single
    // sub-batch runs on the caller's stream: no helper streams, no events.
    const bool fork = L.nsplit >= 2;
    if (fork) {
        if (!ctx->aux_ready) {
            for (int i = 0; i < 4; ++i) {
                UWIE_HIP_CHECK(hipStreamCreateWithFlags(&ctx->aux[i], hipStreamNonBlocking));
                UWIE_HIP_CHECK(hipEventCreateWithFlags(&ctx->join[i], hipEventDisableTiming));
            }
            UWIE_HIP_CHECK(hipEventCreateWithFlags(&ctx->fork, hipEventDisableTiming));
            ctx->aux_ready = true;
        }
        UWIE_HIP_CHECK(hipEventRecord(ctx->fork, st));
    }
    for (int i = 0; i < L.nsplit; ++i) {
        hipStream_t sti = fork ? ctx->aux[i] : st;
        if (fork) UWIE_HIP_CHECK(hipStreamWaitEvent(sti, ctx->fork, 0));
        const size_t first = (size_t)L.start[i] * H * W * 3;
        UWIE_TRY(run_enhance(ctx, d_in + first, Shape{L.cnt[i], H, W}, L.plan[i], p, L.P[i], d_out_u8 ? d_out_u8 + first : nullptr,
                             d_out_f32 ? d_out_f32 + first : nullptr, nullptr, sti));
        if (fork) UWIE_HIP_CHECK(hipEventRecord(ctx->join[i], sti));
    }
    for (int i = 0; fork && i < L.nsplit; ++i) UWIE_HIP_CHECK(hipStreamWaitEvent(st, ctx->join[i], 0));
    return UWIE_OK;
}

int uwie_enhance_u8_f64(uwie_ctx *ctx, const uint8_t *d_in, uint8_t *d_out_u8, double *d_out_f64, int batch, int H, int W,
                        const uwie_params *p, void *d_workspace, size_t workspace_bytes, void *stream)
{
    UWIE_REQUIRE(ctx && d_in && d_out_f64, "enhance_f64: NULL context or image pointer");
    UWIE_SCOPE(ctx);
    UWIE_CHECK_SHAPE(batch, H, W);
    UWIE_TRY(check_params(p));
    UWIE_REQUIRE(p->surface == UWIE_SURFACE_DICT, "enhance_f64: float64 images are the dict surface's (ES:247,307,345)");
    size_t need;
    const EnhanceLayout L = enhance_layout(d_workspace, workspace_bytes, Shape{batch, H, W}, p, false, &need);
    UWIE_CHECK_WS(need);
    ctx->last_enhance_f64 = true;  // (the whole batch in one layout: uwie_enhance_percentiles reads that one)
    return run_enhance(ctx, d_in, Shape{batch, H, W}, L.plan[0], p, L.P[0], d_out_u8, nullptr, d_out_f64, (hipStream_t)stream);
}

size_t uwie_workspace_bytes_float(int batch, int H, int W, const uwie_params *p, int elem_bytes)
{
    if (!shape_ok(batch, H, W) || !p || (elem_bytes != 4 && elem_bytes != 8)) return 0;
    return elem_bytes == 4 ? float_ws_bytes<float>(batch, H, W, p) : float_ws_bytes<double>(batch, H, W, p);
}

int uwie_enhance_f32(uwie_ctx *ctx, const float *d_img, uint8_t *d_out_u8, float *d_out_f32, double *d_out_f64, int batch, int H, int W,
                     const uwie_params *p, void *d_workspace, size_t workspace_bytes, void *stream)
{
    UWIE_REQUIRE(ctx && d_img && (d_out_u8 || d_out_f32 || d_out_f64), "enhance_f32: NULL context or image pointer");
    UWIE_SCOPE(ctx);
    UWIE_CHECK_SHAPE(batch, H, W);
    UWIE_TRY(check_params(p));
    UWIE_REQUIRE(p->dark_patch <= 1, "enhance_f32: dark_patch > 1 is built for u8 frames only (uwie_enhance_u8)");
    const Shape s{batch, H, W};
    Carver c(d_workspace);
    FloatPipe<float> P = carve_float<float>(c, s, p);
    UWIE_CHECK_WS(c.total());
    if (p->surface == UWIE_SURFACE_SIX) {
        UWIE_REQUIRE(!d_out_f64, "enhance_f32: the six_stadigy strategies return float32 images");
        return run_float_six(ctx, d_img, s, p, P, d_out_u8, d_out_f32, (hipStream_t)stream);
    }
    return run_float_dict<float>(ctx, d_img, s, p, P, d_out_u8, d_out_f32, d_out_f64, (hipStream_t)stream);
}

int uwie_enhance_f64(uwie_ctx *ctx, const double *d_img, uint8_t *d_out_u8, double *d_out_f64, int batch, int H, int W,
                     const uwie_params *p, void *d_workspace, size_t workspace_bytes, void *stream)
{
    UWIE_REQUIRE(ctx && d_img && (d_out_u8 || d_out_f64), "enhance_f64: NULL context or image pointer");
    UWIE_SCOPE(ctx);
    UWIE_CHECK_SHAPE(batch, H, W);
    UWIE_TRY(check_params(p));
    UWIE_REQUIRE(p->surface == UWIE_SURFACE_DICT, "enhance_f64: float64 images are the dict surface's (six_stadigy.py works on float32, S6:406)");
    UWIE_REQUIRE(p->dark_patch <= 1, "enhance_f64: dark_patch > 1 is built for u8 frames only (uwie_enhance_u8_f64)");
    const Shape s{batch, H, W};
    Carver c(d_workspace);
    FloatPipe<double> P = carve_float<double>(c, s, p);
    UWIE_CHECK_WS(c.total());
    return run_float_dict<double>(ctx, d_img, s, p, P, d_out_u8, nullptr, d_out_f64, (hipStream_t)stream);
}

int uwie_color_correct_f32(uwie_ctx *ctx, const float *d_img, const int32_t *d_kind, float *d_out, int batch, int H, int W, void *stream)
{
    UWIE_REQUIRE(ctx && d_img && d_kind && d_out, "color_correct_f32: NULL pointer");
    UWIE_SCOPE(ctx);
    UWIE_CHECK_SHAPE(batch, H, W);
    return launch_float_prepare<float>(d_img, d_kind, d_out, nullptr, Shape{batch, H, W}, (hipStream_t)stream);
}

int uwie_cast_classify_f32(uwie_ctx *ctx, const float *d_img, int batch, int H, int W, int32_t *d_kind, float *d_mean_rgb, void *stream)
{
    UWIE_REQUIRE(ctx && d_img && (d_kind || d_mean_rgb), "cast_classify_f32: NULL pointer");
    UWIE_SCOPE(ctx);
    UWIE_CHECK_SHAPE(batch, H, W);
    return launch_float_cast_classify<float>(d_img, Shape{batch, H, W}, d_kind, d_mean_rgb, (hipStream_t)stream);
}

int uwie_enhance_all_u8(uwie_ctx *ctx, const uint8_t *d_in, uint8_t *d_out_u8, int32_t *d_kind, int batch, int H, int W,
                        const uwie_params *p6, void *d_workspace, size_t workspace_bytes, void *stream)
{
    UWIE_REQUIRE(ctx && d_in && d_out_u8, "enhance_all: NULL context or image pointer");
    UWIE_SCOPE(ctx);
    UWIE_CHECK_SHAPE(batch, H, W);
    uwie_params P6[6];
    for (int k = 0; k < 6; ++k) {
        if (p6) P6[k] = p6[k];
        else UWIE_TRY(uwie_params_init(&P6[k], UWIE_SURFACE_SIX, k + 1));
        UWIE_TRY(check_params(&P6[k]));
        UWIE_REQUIRE(P6[k].surface == UWIE_SURFACE_SIX && P6[k].strategy == k + 1, "enhance_all: params must be strategies 1..6 in order");
        UWIE_REQUIRE(P6[k].cast_correct == P6[0].cast_correct && P6[k].forced_cast == P6[0].forced_cast &&
                         P6[k].gray_shift == P6[0].gray_shift && P6[k].min_size == P6[0].min_size,
                     "enhance_all: the six parameter sets must agree on the shared stages (cast, gray, quadtree)");
    }
    const Shape s{batch, H, W};
    Carver c(d_workspace);
    EnhancePlan six[6];
    const Pipe P = carve_pipe(c, s, plan_enhance_all(s, P6, six));  // a dehazing layout sized for the most demanding of the six sets
    UWIE_CHECK_WS(c.total());
    hipStream_t st = (hipStream_t)stream;
    const int32_t *kind = nullptr;
    UWIE_TRY(six_cast(ctx, d_in, s, six[0], &P6[0], P, &kind, st));
    if (d_kind) {
        if (kind) UWIE_HIP_CHECK(hipMemcpyAsync(d_kind, kind, sizeof(int32_t) * batch, hipMemcpyDeviceToDevice, st));
        else UWIE_HIP_CHECK(hipMemsetAsync(d_kind, 0, sizeof(int32_t) * batch, st));
    }
    UWIE_TRY(six_airlight(ctx, d_in, kind, s, six[0], &P6[0], P, st));
    const size_t out_stride = (size_t)batch * H * W * 3;
    for (int k = 0; k < 6; ++k) {
        uint8_t *out = d_out_u8 + (size_t)k * out_stride;
        if (k < 3) UWIE_TRY(six_dehaze_tail(ctx, d_in, kind, s, six[k], &P6[k], P, out, nullptr, st));
        else UWIE_TRY(launch_code_strategy(ctx, d_in, kind, s, &P6[k], out, nullptr, P.scratch, st));
    }
    return UWIE_OK;
}

// ---- main.py:118-146: every strategy of Config.STRATEGIES on the frame, comprehensive_assessment of each result, the best one
namespace {
struct SelectBufs {
    void *pipe;
    size_t pipe_bytes;
    uint8_t *all;
    float *f32;
    void *qa;
};
SelectBufs carve_select(Carver &c, Shape s, const uwie_params *ps, int n, bool own_all)
{
    SelectBufs b{};
    for (int k = 0; k < n; ++k) {
        Carver ck(nullptr);
        carve_pipe(ck, s, plan_enhance(s, &ps[k]));
        if (ck.total() > b.pipe_bytes) b.pipe_bytes = ck.total();
    }
    b.pipe = c.take<char>(b.pipe_bytes);
    b.all = own_all ? c.take<uint8_t>((size_t)n * s.B * s.npx() * 3) : nullptr;
    b.f32 = c.take<float>((size_t)s.B * s.npx() * 3);
    b.qa = c.take<char>(quality_ws_bytes(s));
    return b;
}
}  // namespace

size_t uwie_workspace_bytes_select(int batch, int H, int W, const uwie_params *ps, int n, int with_outputs)
{
    if (!shape_ok(batch, H, W) || !ps || n < 1 || n > 16) return 0;
    Carver c(nullptr);
    carve_select(c, Shape{batch, H, W}, ps, n, !with_outputs);
    return c.total();
}

int uwie_select_best_u8(uwie_ctx *ctx, const uint8_t *d_in, int batch, int H, int W, const uwie_params *ps, int n,
                        const double *weights8, uint8_t *d_best_u8, int32_t *d_best, double *d_scores, uint8_t *d_all_u8,
                        void *d_workspace, size_t workspace_bytes, void *stream)
{
    UWIE_REQUIRE(ctx && d_in && ps && d_best && d_scores, "select_best: NULL pointer");
    UWIE_SCOPE(ctx);
    UWIE_CHECK_SHAPE(batch, H, W);
    UWIE_REQUIRE(n >= 1 && n <= 16, "select_best: 1 .. 16 strategies");
    for (int k = 0; k < n; ++k) UWIE_TRY(check_params(&ps[k]));
    static const double kDefault[8] = {0.20, 0.20, 0.15, 0.15, 0.10, 0.10, 0.05, 0.05};  // quality_assessment.py:229-238
    const Shape s{batch, H, W};
    Carver c(d_workspace);
    SelectBufs sb = carve_select(c, s, ps, n, d_all_u8 == nullptr);
    UWIE_CHECK_WS(c.total());
    hipStream_t st = (hipStream_t)stream;
    uint8_t *all = d_all_u8 ? d_all_u8 : sb.all;
    const size_t frame_set = (size_t)batch * H * W * 3;
    int shared_with = -1;  // the dict dehazing set whose gray plane / atmospheric light are still in the workspace
    for (int k = 0; k < n; ++k) {
        const uwie_params *p = &ps[k];
        Carver ck(sb.pipe);
        const EnhancePlan e = plan_enhance(s, p);
        const Pipe P = carve_pipe(ck, s, e);
        uint8_t *out = all + (size_t)k * frame_set;
        // one quadtree for all the dict dehazing sets that follow each other with the same leaf size and gray coefficients
        const bool have = e.pipeline == EP_DICT_DEHAZE && shared_with >= 0 && ps[shared_with].min_size == p->min_size &&
                          ps[shared_with].gray_shift == p->gray_shift && ps[shared_with].gf_exact == p->gf_exact;
        UWIE_TRY(run_enhance(ctx, d_in, s, e, p, P, out, sb.f32, nullptr, st, have));
        if (e.pipeline != EP_DICT_DEHAZE) shared_with = -1;
        else if (!have) shared_with = k;
        // (img * 255).astype(uint8) is what every score but colourfulness starts from; that one takes the float image
        UWIE_TRY(launch_quality_scores(ctx, out, sb.f32, s, p->gray_shift, weights8 ? weights8 : kDefault,
                                       d_scores + (size_t)k * batch * 9, sb.qa, st));
    }
    return launch_pick_best(d_scores, n, s, 9, 8, all, d_best, d_best_u8, st);
}

// The two enhancement modules (k_diffenh.hip): map is UWIE_LOSS_VGG (vgg_16_UIE.DifferentiableEnhancement) or
// UWIE_LOSS_GATED (deep_learning_parameters.DifferentiableEnhancement, whose flags are reserved: 0).
// The common start of their forwards: the module's sorted positions, then the selection.  *os = the order statistics.
static int module_select(uwie_ctx *ctx, int map, const float *d_img, int planar, Shape s, const float *d_params, void *sel_ws,
                         hipStream_t st, const float **os)
{
    SelectPlan plan;
    if (map == UWIE_LOSS_VGG) UWIE_TRY(select_begin_stretch_ranks(s, d_params, 4, sel_ws, st, &plan));
    else UWIE_TRY(select_begin_gated_ranks(s, d_params, 4, ctx->d_status, sel_ws, st, &plan));
    UWIE_TRY(select_run(plan, d_img, planar, s, false, st));
    *os = (const float *)plan.os;
    return UWIE_OK;
}

// a module forward after its entry point's NULL check (who: the entry point in messages; d_saved: the _save_f32 form)
static int module_fwd(const char *who, uwie_ctx *ctx, int map, const float *d_img, float *d_out, int batch, int H, int W, int planar,
                      const float *d_params, int flags, float *d_saved, void *d_workspace, size_t workspace_bytes, void *stream)
{
    UWIE_SCOPE(ctx);
    UWIE_CHECK_SHAPE(batch, H, W);
    UWIE_TRY(module_flags_check(who, map, flags));
    const Shape s{batch, H, W};
    UWIE_CHECK_WS(select_ws_bytes(s));
    hipStream_t st = (hipStream_t)stream;
    const float *os = nullptr;
    UWIE_TRY(module_select(ctx, map, d_img, planar ? 1 : 0, s, d_params, d_workspace, st, &os));
    if (map == UWIE_LOSS_VGG) return launch_diff_enhance(d_img, planar ? 1 : 0, s, d_params, flags, os, d_out, st, d_saved);
    return launch_diff_gated(d_img, planar ? 1 : 0, s, d_params, os, d_out, st, d_saved);
}

// a module backward after its entry point's NULL check
static int module_bwd(const char *who, uwie_ctx *ctx, int map, const float *d_img, const float *d_params, int flags, int planar,
                      int batch, int H, int W, const float *d_saved, const float *d_grad_out, float *d_grad_img, float *d_grad_params,
                      void *d_workspace, size_t workspace_bytes, void *stream)
{
    UWIE_SCOPE(ctx);
    UWIE_CHECK_SHAPE(batch, H, W);
    UWIE_TRY(module_flags_check(who, map, flags));
    UWIE_REQUIRE_F((const void *)d_grad_img != (const void *)d_img && (const void *)d_grad_img != (const void *)d_grad_out,
                   "%s: d_grad_img must not alias d_img or d_grad_out", who);
    const Shape s{batch, H, W};
    UWIE_CHECK_WS(diff_enhance_bwd_ws_bytes(s));
    return launch_module_bwd(map, d_img, planar ? 1 : 0, s, d_params, flags, d_saved, nullptr, d_grad_out, nullptr, d_grad_img,
                             d_grad_params, d_workspace, (hipStream_t)stream);
}

// a module for u8 frames in the byte domain (k_diff_u8.hip).  Every argument check needs no device and runs ahead of the scope.
static int module_u8(const char *who, uwie_ctx *ctx, int map, const uint8_t *d_in, uint8_t *d_out_u8, float *d_out_f32, int batch,
                     int H, int W, const float *d_params, int flags, float *d_saved, void *d_workspace, size_t workspace_bytes,
                     void *stream)
{
    const bool gated = map == UWIE_LOSS_GATED;
    UWIE_REQUIRE_F(ctx && d_in && d_params, "%s: NULL pointer", who);
    UWIE_REQUIRE_F(d_out_u8 || d_out_f32, "%s: at least one of d_out_u8, d_out_f32", who);
    UWIE_REQUIRE_F(((uintptr_t)d_in & 3) == 0, "%s: d_in must be 4-byte aligned", who);  // k_frame_hist reads dwords
    UWIE_CHECK_SHAPE(batch, H, W);
    UWIE_REQUIRE_F(!gated || batch <= 65535, "%s: batch is at most 65535", who);  // k_dg8_table's grid: one row per image
    UWIE_TRY(module_flags_check(who, map, flags));
    const Shape s{batch, H, W};
    UWIE_CHECK_WS(gated ? diff_gated_u8_ws_bytes(batch) : diff_u8_ws_bytes(s));
    UWIE_SCOPE(ctx);
    hipStream_t st = (hipStream_t)stream;
    if (gated) return launch_diff_gated_u8(d_in, s, d_params, ctx->d_status, d_out_u8, d_out_f32, d_saved, d_workspace, st);
    return launch_diff_enhance_u8(d_in, s, d_params, flags, d_out_u8, d_out_f32, d_saved, d_workspace, st);
}

int uwie_diff_enhance_f32(uwie_ctx *ctx, const float *d_img, float *d_out, int batch, int H, int W, int planar,
                          const float *d_params, int flags, void *d_workspace, size_t workspace_bytes, void *stream)
{
    UWIE_REQUIRE(ctx && d_img && d_out && d_params, "diff_enhance: NULL pointer");
    return module_fwd("diff_enhance", ctx, UWIE_LOSS_VGG, d_img, d_out, batch, H, W, planar, d_params, flags, nullptr, d_workspace,
                      workspace_bytes, stream);
}

int uwie_diff_enhance_save_f32(uwie_ctx *ctx, const float *d_img, float *d_out, int batch, int H, int W, int planar,
                               const float *d_params, int flags, float *d_saved, void *d_workspace, size_t workspace_bytes,
                               void *stream)
{
    UWIE_REQUIRE(ctx && d_img && d_out && d_params && d_saved, "diff_enhance_save: NULL pointer");
    return module_fwd("diff_enhance_save", ctx, UWIE_LOSS_VGG, d_img, d_out, batch, H, W, planar, d_params, flags, d_saved,
                      d_workspace, workspace_bytes, stream);
}

size_t uwie_diff_enhance_bwd_workspace_bytes(int batch, int H, int W)
{
    if (!shape_ok(batch, H, W)) return 0;
    return diff_enhance_bwd_ws_bytes(Shape{batch, H, W});
}

int uwie_diff_enhance_bwd_f32(uwie_ctx *ctx, const float *d_img, const float *d_params, int flags, int planar, int batch,
                              int H, int W, const float *d_saved, const float *d_grad_out, float *d_grad_img,
                              float *d_grad_params, void *d_workspace, size_t workspace_bytes, void *stream)
{
    UWIE_REQUIRE(ctx && d_img && d_params && d_saved && d_grad_out && d_grad_params, "diff_enhance_bwd: NULL pointer");
    return module_bwd("diff_enhance_bwd", ctx, UWIE_LOSS_VGG, d_img, d_params, flags, planar, batch, H, W, d_saved, d_grad_out,
                      d_grad_img, d_grad_params, d_workspace, workspace_bytes, stream);
}

size_t uwie_workspace_bytes_diff_u8(int batch, int H, int W)
{
    if (!shape_ok(batch, H, W)) return 0;
    return diff_u8_ws_bytes(Shape{batch, H, W});
}

int uwie_diff_enhance_u8(uwie_ctx *ctx, const uint8_t *d_in, uint8_t *d_out_u8, float *d_out_f32, int batch, int H, int W,
                         const float *d_params, int flags, float *d_saved, void *d_workspace, size_t workspace_bytes, void *stream)
{
    return module_u8("diff_enhance_u8", ctx, UWIE_LOSS_VGG, d_in, d_out_u8, d_out_f32, batch, H, W, d_params, flags, d_saved,
                     d_workspace, workspace_bytes, stream);
}

size_t uwie_workspace_bytes_diff_gated_u8(int batch)
{
    if (batch < 1) return 0;
    return diff_gated_u8_ws_bytes(batch);
}

int uwie_diff_gated_u8(uwie_ctx *ctx, const uint8_t *d_in, uint8_t *d_out_u8, float *d_out_f32, int batch, int H, int W,
                       const float *d_params, int flags, float *d_saved, void *d_workspace, size_t workspace_bytes, void *stream)
{
    return module_u8("diff_gated_u8", ctx, UWIE_LOSS_GATED, d_in, d_out_u8, d_out_f32, batch, H, W, d_params, flags, d_saved,
                     d_workspace, workspace_bytes, stream);
}

int uwie_diff_gated_f32(uwie_ctx *ctx, const float *d_img, float *d_out, int batch, int H, int W, int planar,
                        const float *d_params, int flags, void *d_workspace, size_t workspace_bytes, void *stream)
{
    UWIE_REQUIRE(ctx && d_img && d_out && d_params, "diff_gated: NULL pointer");
    return module_fwd("diff_gated", ctx, UWIE_LOSS_GATED, d_img, d_out, batch, H, W, planar, d_params, flags, nullptr, d_workspace,
                      workspace_bytes, stream);
}

int uwie_diff_gated_save_f32(uwie_ctx *ctx, const float *d_img, float *d_out, int batch, int H, int W, int planar,
                             const float *d_params, int flags, float *d_saved, void *d_workspace, size_t workspace_bytes,
                             void *stream)
{
    UWIE_REQUIRE(ctx && d_img && d_out && d_params && d_saved, "diff_gated_save: NULL pointer");
    return module_fwd("diff_gated_save", ctx, UWIE_LOSS_GATED, d_img, d_out, batch, H, W, planar, d_params, flags, d_saved,
                      d_workspace, workspace_bytes, stream);
}

size_t uwie_diff_gated_bwd_workspace_bytes(int batch, int H, int W)
{
    return uwie_diff_enhance_bwd_workspace_bytes(batch, H, W);  // the same partials
}

int uwie_diff_gated_bwd_f32(uwie_ctx *ctx, const float *d_img, const float *d_params, int flags, int planar, int batch, int H,
                            int W, const float *d_saved, const float *d_grad_out, float *d_grad_img, float *d_grad_params,
                            void *d_workspace, size_t workspace_bytes, void *stream)
{
    UWIE_REQUIRE(ctx && d_img && d_params && d_saved && d_grad_out && d_grad_params, "diff_gated_bwd: NULL pointer");
    return module_bwd("diff_gated_bwd", ctx, UWIE_LOSS_GATED, d_img, d_params, flags, planar, batch, H, W, d_saved, d_grad_out,
                      d_grad_img, d_grad_params, d_workspace, workspace_bytes, stream);
}

// ReferenceLoss: the forward workspace holds the selection and the loss partials; the backward's is the module backward's
static size_t ref_loss_fwd_ws_bytes(Shape s)
{
    Carver c(nullptr);
    c.take<char>(select_ws_bytes(s));
    c.take<char>(refloss_ws_bytes(s));
    return c.total();
}

size_t uwie_ref_loss_workspace_bytes(int batch, int H, int W)
{
    if (!shape_ok(batch, H, W)) return 0;
    const Shape s{batch, H, W};
    return std::max(ref_loss_fwd_ws_bytes(s), diff_enhance_bwd_ws_bytes(s));
}

static int ref_loss_check_map(int map, const float *d_params, const float *d_saved, int flags)
{
    UWIE_REQUIRE(map == UWIE_LOSS_IDENTITY || map == UWIE_LOSS_VGG || map == UWIE_LOSS_GATED,
                 "ref_loss: map is UWIE_LOSS_IDENTITY, UWIE_LOSS_VGG or UWIE_LOSS_GATED");
    if (map == UWIE_LOSS_IDENTITY) return UWIE_OK;
    UWIE_REQUIRE(d_params && d_saved, "ref_loss: NULL pointer (d_params, d_saved)");
    return module_flags_check("ref_loss", map, flags, true);
}

int uwie_ref_loss_f32(uwie_ctx *ctx, int map, const float *d_img, const float *d_params, int flags, int planar, int batch, int H,
                      int W, const float *d_ref, float *d_out, float *d_saved, float *d_loss, void *d_workspace,
                      size_t workspace_bytes, void *stream)
{
    UWIE_REQUIRE(ctx && d_img && d_ref && d_loss, "ref_loss: NULL pointer");
    UWIE_TRY(ref_loss_check_map(map, d_params, d_saved, flags));
    UWIE_CHECK_SHAPE(batch, H, W);
    UWIE_REQUIRE((const void *)d_out != (const void *)d_img && (const void *)d_out != (const void *)d_ref,
                 "ref_loss: d_out must not alias d_img or d_ref");
    const Shape s{batch, H, W};
    UWIE_CHECK_WS(ref_loss_fwd_ws_bytes(s));
    UWIE_SCOPE(ctx);
    hipStream_t st = (hipStream_t)stream;
    Carver c(d_workspace);
    void *sel_ws = c.take<char>(select_ws_bytes(s));
    void *loss_ws = c.take<char>(refloss_ws_bytes(s));
    const float *os = nullptr;
    if (map != UWIE_LOSS_IDENTITY) {
        UWIE_TRY(module_select(ctx, map, d_img, planar ? 1 : 0, s, d_params, sel_ws, st, &os));
    } else {
        d_out = nullptr;
        d_saved = nullptr;
    }
    return launch_refloss(map, d_img, planar ? 1 : 0, s, d_params, flags, os, d_ref, d_out, d_saved, d_loss, loss_ws, st);
}

int uwie_ref_loss_bwd_f32(uwie_ctx *ctx, int map, const float *d_img, const float *d_params, int flags, int planar, int batch,
                          int H, int W, const float *d_saved, const float *d_ref, const float *d_grad_out,
                          const float *d_grad_loss, float *d_grad_img, float *d_grad_params, void *d_workspace,
                          size_t workspace_bytes, void *stream)
{
    UWIE_REQUIRE(ctx && d_img && d_ref && d_grad_loss, "ref_loss_bwd: NULL pointer");
    UWIE_TRY(ref_loss_check_map(map, d_params, d_saved, flags));
    UWIE_REQUIRE(map == UWIE_LOSS_IDENTITY ? d_grad_img != nullptr : d_grad_params != nullptr,
                 "ref_loss_bwd: NULL pointer (identity: d_grad_img; vgg / gated: d_grad_params)");
    UWIE_CHECK_SHAPE(batch, H, W);
    UWIE_REQUIRE(!d_grad_img || ((const void *)d_grad_img != (const void *)d_img && (const void *)d_grad_img != (const void *)d_ref &&
                                 (const void *)d_grad_img != (const void *)d_grad_out),
                 "ref_loss_bwd: d_grad_img must not alias d_img, d_ref or d_grad_out");
    const Shape s{batch, H, W};
    if (map != UWIE_LOSS_IDENTITY) UWIE_CHECK_WS(diff_enhance_bwd_ws_bytes(s));
    UWIE_SCOPE(ctx);
    return launch_refloss_bwd(map, d_img, planar ? 1 : 0, s, d_params, flags, d_saved, d_ref, d_grad_out, d_grad_loss, d_grad_img,
                              d_grad_params, d_workspace, (hipStream_t)stream);
}

// PerceptualLoss (k_vgg.hip)
struct uwie_vgg : Handle<VggNet> {};

static bool perceptual_shape_ok(int batch, int H, int W)
{
    return shape_ok(batch, H, W) && H >= 4 && W >= 4 && (long long)batch * H * W <= (1ll << 28);
}

int uwie_vgg_create(uwie_ctx *ctx, const float *d_params, int precision, uwie_vgg **out_vgg)
{
    UWIE_REQUIRE(ctx && d_params && out_vgg, "vgg_create: NULL pointer");
    *out_vgg = nullptr;
    UWIE_REQUIRE(precision == UWIE_VGG_F32 || precision == UWIE_VGG_F16, "vgg_create: precision is UWIE_VGG_F32 or UWIE_VGG_F16");
    static_assert(UWIE_VGG_PARAMS > 0, "");
    if (vgg_param_count() != (size_t)UWIE_VGG_PARAMS) {
        set_error("vgg_create: internal parameter count %zu differs from UWIE_VGG_PARAMS", vgg_param_count());
        return UWIE_E_INVALID;
    }
    UWIE_SCOPE(ctx);
    void *blob = nullptr;
    UWIE_HIP_CHECK(hipMalloc(&blob, vgg_blob_bytes(precision)));
    VggNet net{};
    UWIE_TRY(pack_finish(vgg_pack(d_params, precision, blob, &net, nullptr), "vgg_create", [&] { (void)hipFree(blob); }));
    *out_vgg = new uwie_vgg{{ctx->device, net, blob}};
    return UWIE_OK;
}

void uwie_vgg_destroy(uwie_vgg *vgg) { handle_destroy(vgg); }

size_t uwie_perceptual_workspace_bytes(int batch, int H, int W, int precision)
{
    if (!perceptual_shape_ok(batch, H, W) || (precision != UWIE_VGG_F32 && precision != UWIE_VGG_F16)) return 0;
    return perceptual_ws_bytes(Shape{batch, H, W}, precision);
}

static int perceptual_check(uwie_ctx *ctx, const uwie_vgg *vgg, int batch, int H, int W)
{
    UWIE_REQUIRE(vgg->device == ctx->device, "perceptual: the network lives on another device");
    UWIE_REQUIRE(shape_ok(batch, H, W) && (long long)batch * H * W <= (1ll << 28), "perceptual: batch/H/W out of range");
    if (H < 4 || W < 4) {
        set_error("perceptual: H and W must be >= 4 (got %d x %d): a max-pool output would be empty", H, W);
        return UWIE_E_INVALID;
    }
    return UWIE_OK;
}

int uwie_perceptual_f32(uwie_ctx *ctx, const uwie_vgg *vgg, const float *d_pred, const float *d_target, int batch, int H, int W,
                        float *d_loss, void *d_workspace, size_t workspace_bytes, void *stream)
{
    UWIE_REQUIRE(ctx && vgg && d_pred && d_target && d_loss, "perceptual: NULL pointer");
    UWIE_TRY(perceptual_check(ctx, vgg, batch, H, W));
    const Shape s{batch, H, W};
    UWIE_CHECK_WS(perceptual_ws_bytes(s, vgg->net.precision));
    UWIE_SCOPE(ctx);
    return launch_perceptual(vgg->net, d_pred, d_target, s, d_loss, d_workspace, (hipStream_t)stream);
}

int uwie_perceptual_bwd_f32(uwie_ctx *ctx, const uwie_vgg *vgg, int batch, int H, int W, const float *d_grad_loss, float *d_grad_pred,
                            void *d_workspace, size_t workspace_bytes, void *stream)
{
    UWIE_REQUIRE(ctx && vgg && d_grad_loss && d_grad_pred, "perceptual_bwd: NULL pointer");
    UWIE_TRY(perceptual_check(ctx, vgg, batch, H, W));
    const Shape s{batch, H, W};
    UWIE_CHECK_WS(perceptual_ws_bytes(s, vgg->net.precision));
    UWIE_SCOPE(ctx);
    return launch_perceptual_bwd(vgg->net, s, d_grad_loss, d_grad_pred, d_workspace, (hipStream_t)stream);
}

// ImprovedVGGParameterNet (k_param_net.hip)
struct uwie_param_net : Handle<ParamNet> {};

static bool param_net_shape_ok(int batch, int H, int W)
{
    return shape_ok(batch, H, W) && H >= 8 && W >= 8 && (long long)batch * H * W <= (1ll << 28);
}

int uwie_param_net_create(uwie_ctx *ctx, const float *d_params, int use_features, uwie_param_net **out_net)
{
    UWIE_REQUIRE(ctx && d_params && out_net, "param_net_create: NULL pointer");
    *out_net = nullptr;
    const int uf = use_features ? 1 : 0;
    if (param_net_count(uf) != (size_t)UWIE_PARAM_NET_PARAMS(uf)) {
        set_error("param_net_create: internal parameter count %zu differs from UWIE_PARAM_NET_PARAMS", param_net_count(uf));
        return UWIE_E_INVALID;
    }
    UWIE_SCOPE(ctx);
    void *blob = nullptr, *scratch = nullptr;
    UWIE_HIP_CHECK(hipMalloc(&blob, param_net_blob_bytes(uf)));
    hipError_t e = hipMalloc(&scratch, param_net_scratch_floats() * sizeof(float));
    if (e != hipSuccess) {
        (void)hipFree(blob);
        set_error("param_net_create: %s", hipGetErrorString(e));
        return UWIE_E_HIP;
    }
    ParamNet net{};
    const int rc = pack_finish(param_net_pack(d_params, uf, blob, static_cast<float *>(scratch), &net, nullptr),
                               "param_net_create", [&] { (void)hipFree(blob); });
    (void)hipFree(scratch);  // the data-gradient copy of conv4_x: not needed for inference
    UWIE_TRY(rc);
    *out_net = new uwie_param_net{{ctx->device, net, blob}};
    return UWIE_OK;
}

void uwie_param_net_destroy(uwie_param_net *net) { handle_destroy(net); }

size_t uwie_param_net_workspace_bytes(int batch, int H, int W)
{
    if (!param_net_shape_ok(batch, H, W)) return 0;
    return param_net_ws_bytes(Shape{batch, H, W});
}

int uwie_param_net_f32(uwie_ctx *ctx, const uwie_param_net *net, const float *d_img, const float *d_features, int batch, int H, int W,
                       float *d_out, float *d_pooled, void *d_workspace, size_t workspace_bytes, void *stream)
{
    UWIE_REQUIRE(ctx && net && d_img && d_out, "param_net: NULL pointer");
    UWIE_REQUIRE(net->device == ctx->device, "param_net: the network lives on another device");
    UWIE_REQUIRE(shape_ok(batch, H, W) && (long long)batch * H * W <= (1ll << 28), "param_net: batch/H/W out of range");
    if (H < 8 || W < 8) {
        set_error("param_net: H and W must be >= 8 (got %d x %d): pool3's output would be empty", H, W);
        return UWIE_E_INVALID;
    }
    UWIE_REQUIRE(d_features || net->net.din == 1024, "param_net: a use_features network needs d_features [batch][79]");
    const Shape s{batch, H, W};
    UWIE_CHECK_WS(param_net_ws_bytes(s));
    UWIE_SCOPE(ctx);
    return launch_param_net(net->net, d_img, d_features, s, d_out, d_pooled, d_workspace, (hipStream_t)stream);
}

// ParameterPredictor (k_param_net.hip)
struct uwie_mlp : Handle<Mlp> {};

static bool mlp_dims_ok(int F, int Hd, int nb)
{
    return F >= 1 && F <= 1152 && Hd >= 2 && Hd <= 1152 && Hd % 2 == 0 && nb >= 0 && nb <= 64;
}

int uwie_mlp_create(uwie_ctx *ctx, const float *d_params, int feature_dim, int hidden_dim, int num_blocks, uwie_mlp **out_net)
{
    UWIE_REQUIRE(ctx && d_params && out_net, "mlp_create: NULL pointer");
    *out_net = nullptr;
    UWIE_REQUIRE(mlp_dims_ok(feature_dim, hidden_dim, num_blocks),
                 "mlp_create: feature_dim 1 .. 1152, hidden_dim even 2 .. 1152, num_blocks 0 .. 64");
    UWIE_SCOPE(ctx);
    void *blob = nullptr;
    UWIE_HIP_CHECK(hipMalloc(&blob, mlp_count(feature_dim, hidden_dim, num_blocks) * sizeof(float)));
    Mlp net{};
    UWIE_TRY(pack_finish(mlp_pack(d_params, feature_dim, hidden_dim, num_blocks, static_cast<float *>(blob), &net, nullptr),
                         "mlp_create", [&] { (void)hipFree(blob); }));
    *out_net = new uwie_mlp{{ctx->device, net, blob}};
    return UWIE_OK;
}

void uwie_mlp_destroy(uwie_mlp *net) { handle_destroy(net); }

size_t uwie_mlp_workspace_bytes(int batch, int hidden_dim)
{
    if (batch < 1 || batch > kMlpEvalBatch || !mlp_dims_ok(1, hidden_dim, 0)) return 0;
    return mlp_ws_bytes(batch, hidden_dim);
}

// the eval forward of a network or of a trainer's current parameters
static int mlp_eval(const Mlp &net, uwie_ctx *ctx, const void *d_features, int features_are_f64, int batch, float *d_out,
                    void *d_workspace, size_t workspace_bytes, void *stream)
{
    UWIE_CHECK_WS(mlp_ws_bytes(batch, net.H));
    UWIE_SCOPE(ctx);
    return launch_mlp(net, d_features, features_are_f64 != 0, batch, d_out, d_workspace, (hipStream_t)stream);
}

int uwie_mlp_forward(uwie_ctx *ctx, const uwie_mlp *net, const void *d_features, int features_are_f64, int batch, float *d_out,
                     void *d_workspace, size_t workspace_bytes, void *stream)
{
    UWIE_TRY(mlp_rows_check("mlp_forward", ctx, net, d_features, features_are_f64, batch, false, d_out, "d_out"));
    return mlp_eval(net->net, ctx, d_features, features_are_f64, batch, d_out, d_workspace, workspace_bytes, stream);
}

// EndToEndTrainer's training step (k_mlp_train.hip)
struct uwie_mlp_trainer {
    int device;
    Mlp net;            // device pointers into arrays[UWIE_TRAINER_PARAMS]
    float *arrays[4];   // parameters, gradients, exp_avg, exp_avg_sq in the packed order (mlp_pack)
    double *partial;    // the norm's per-block sums
    long long step;     // Adam steps taken
    int fwd_batch;      // the batch of the last train forward (0: none) and its dropout scale
    float fwd_scale;
};

static void trainer_free(uwie_mlp_trainer *tr)
{
    for (float *a : tr->arrays) (void)hipFree(a);
    (void)hipFree(tr->partial);
    delete tr;
}

int uwie_mlp_trainer_create(uwie_ctx *ctx, const float *d_params, int feature_dim, int hidden_dim, int num_blocks,
                            uwie_mlp_trainer **out_trainer)
{
    UWIE_REQUIRE(ctx && d_params && out_trainer, "mlp_trainer_create: NULL pointer");
    *out_trainer = nullptr;
    UWIE_REQUIRE(mlp_dims_ok(feature_dim, hidden_dim, num_blocks),
                 "mlp_trainer_create: feature_dim 1 .. 1152, hidden_dim even 2 .. 1152, num_blocks 0 .. 64");
    UWIE_SCOPE(ctx);
    const size_t bytes = mlp_count(feature_dim, hidden_dim, num_blocks) * sizeof(float);
    uwie_mlp_trainer *tr = new uwie_mlp_trainer{};
    tr->device = ctx->device;
    hipError_t e = hipSuccess;
    for (int i = 0; i < 4 && e == hipSuccess; ++i) {
        e = hipMalloc((void **)&tr->arrays[i], bytes);
        if (e == hipSuccess && i > 0) e = hipMemset(tr->arrays[i], 0, bytes);
    }
    if (e == hipSuccess) e = hipMalloc((void **)&tr->partial, mlp_adam_scratch_bytes());
    if (e != hipSuccess) {
        trainer_free(tr);
        set_error("mlp_trainer_create: %s", hipGetErrorString(e));
        return UWIE_E_HIP;
    }
    UWIE_TRY(pack_finish(mlp_pack(d_params, feature_dim, hidden_dim, num_blocks, tr->arrays[UWIE_TRAINER_PARAMS], &tr->net, nullptr),
                         "mlp_trainer_create", [&] { trainer_free(tr); }, ""));
    *out_trainer = tr;
    return UWIE_OK;
}

void uwie_mlp_trainer_destroy(uwie_mlp_trainer *trainer)
{
    if (!trainer) return;
    DeviceGuard on(trainer->device);
    trainer_free(trainer);
}

static bool train_batch_ok(int batch) { return batch >= 1 && batch <= kMlpTrainBatch; }

size_t uwie_mlp_train_workspace_bytes(int batch, int hidden_dim, int num_blocks)
{
    if (!train_batch_ok(batch) || !mlp_dims_ok(1, hidden_dim, num_blocks)) return 0;
    return mlp_train_ws_bytes(batch, hidden_dim, num_blocks);
}

int uwie_mlp_train_forward(uwie_ctx *ctx, uwie_mlp_trainer *trainer, const void *d_features, int features_are_f64, int batch, double p,
                           int mask_mode, uint8_t *d_masks, uint64_t seed, float *d_out, void *d_workspace, size_t workspace_bytes,
                           void *stream)
{
    UWIE_TRY(mlp_rows_check("mlp_train_forward", ctx, trainer, d_features, features_are_f64, batch, true, d_out, "d_out"));
    UWIE_REQUIRE(p >= 0.0 && p < 1.0, "mlp_train_forward: the dropout rate p must lie in [0, 1)");
    UWIE_REQUIRE(mask_mode == UWIE_MASKS_GIVEN || mask_mode == UWIE_MASKS_DRAWN, "mlp_train_forward: mask_mode is UWIE_MASKS_GIVEN or UWIE_MASKS_DRAWN");
    UWIE_REQUIRE(mask_mode == UWIE_MASKS_DRAWN || p == 0.0 || d_masks, "mlp_train_forward: given masks need d_masks");
    const Mlp &net = trainer->net;
    UWIE_CHECK_WS(mlp_train_ws_bytes(batch, net.H, net.nb));
    UWIE_SCOPE(ctx);
    const bool drawn = mask_mode == UWIE_MASKS_DRAWN;
    hipStream_t st = (hipStream_t)stream;
    if (drawn && d_masks && p == 0.0)  // nothing is dropped and no site draws
        UWIE_HIP_CHECK(hipMemsetAsync(d_masks, 1, (size_t)mlp_train_sites(net.nb) * batch * net.H, st));
    UWIE_TRY(launch_mlp_train_forward(net, d_features, features_are_f64 != 0, batch, p, drawn ? nullptr : d_masks,
                                      drawn ? d_masks : nullptr, seed, (uint32_t)trainer->step, d_out, d_workspace, st));
    trainer->fwd_batch = batch;
    trainer->fwd_scale = (float)(1.0 / (1.0 - p));
    return UWIE_OK;
}

int uwie_mlp_backward(uwie_ctx *ctx, uwie_mlp_trainer *trainer, const void *d_features, int features_are_f64, int batch,
                      const float *d_grad_out, void *d_workspace, size_t workspace_bytes, void *stream)
{
    UWIE_TRY(mlp_rows_check("mlp_backward", ctx, trainer, d_features, features_are_f64, batch, true, d_grad_out, "d_grad_out"));
    UWIE_REQUIRE(trainer->fwd_batch == batch, "mlp_backward: no uwie_mlp_train_forward of this batch precedes it");
    const Mlp &net = trainer->net;
    UWIE_CHECK_WS(mlp_train_ws_bytes(batch, net.H, net.nb));
    UWIE_SCOPE(ctx);
    return launch_mlp_backward(net, trainer->arrays[UWIE_TRAINER_GRADS], d_features, features_are_f64 != 0, batch, trainer->fwd_scale,
                               d_grad_out, d_workspace, (hipStream_t)stream);
}

int uwie_mlp_adam_step(uwie_ctx *ctx, uwie_mlp_trainer *trainer, double lr, double beta1, double beta2, double eps, double max_norm,
                       double *d_norm, void *stream)
{
    UWIE_REQUIRE(ctx && trainer, "mlp_adam_step: NULL pointer");
    UWIE_REQUIRE(trainer->device == ctx->device, "mlp_adam_step: the trainer lives on another device");
    UWIE_REQUIRE(lr >= 0.0 && lr < HUGE_VAL && eps >= 0.0 && eps < HUGE_VAL, "mlp_adam_step: lr and eps must be finite and >= 0");
    UWIE_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "mlp_adam_step: the betas must lie in [0, 1)");
    UWIE_REQUIRE(max_norm > 0.0, "mlp_adam_step: max_norm must be > 0");
    UWIE_REQUIRE(((uintptr_t)d_norm & 7) == 0, "mlp_adam_step: d_norm must be 8-byte aligned");
    UWIE_SCOPE(ctx);
    // torch.optim.adam._single_tensor_adam: the bias corrections are Python floats of the step count
    const double t = (double)(trainer->step + 1);
    const double bc1 = 1.0 - pow(beta1, t), bc2 = 1.0 - pow(beta2, t);
    const MlpAdam h{(float)max_norm, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)sqrt(bc2), (float)eps,
                    (float)-(lr / bc1)};
    UWIE_TRY(launch_mlp_adam(trainer->net, trainer->arrays[0], trainer->arrays[1], trainer->arrays[2], trainer->arrays[3],
                             trainer->partial, h, d_norm, (hipStream_t)stream));
    trainer->step += 1;
    return UWIE_OK;
}

static int trainer_copy(uwie_mlp_trainer *tr, int which, float *d_buf, bool get, const char *who)
{
    if (!tr || !d_buf || which < 0 || which > 3 || ((uintptr_t)d_buf & 3)) {
        set_error("%s: NULL or misaligned pointer, or which outside UWIE_TRAINER_PARAMS .. UWIE_TRAINER_EXP_AVG_SQ", who);
        return UWIE_E_INVALID;
    }
    DeviceGuard on(tr->device);
    const Mlp &n = tr->net;
    hipError_t e = hipDeviceSynchronize();  // work on other streams that reads or writes the arrays
    int rc = UWIE_OK;
    if (e == hipSuccess) {
        rc = get ? mlp_repack(tr->arrays[which], d_buf, n.F, n.H, n.nb, true, nullptr)
                 : mlp_repack(d_buf, tr->arrays[which], n.F, n.H, n.nb, false, nullptr);
        if (rc == UWIE_OK) e = hipStreamSynchronize(nullptr);
    }
    if (e != hipSuccess) {
        set_error("%s: %s", who, hipGetErrorString(e));
        return UWIE_E_HIP;
    }
    return rc;
}

int uwie_mlp_trainer_get(uwie_mlp_trainer *trainer, int which, float *d_buf)
{
    return trainer_copy(trainer, which, d_buf, true, "mlp_trainer_get");
}

int uwie_mlp_trainer_set(uwie_mlp_trainer *trainer, int which, const float *d_buf)
{
    return trainer_copy(trainer, which, const_cast<float *>(d_buf), false, "mlp_trainer_set");
}

long long uwie_mlp_trainer_step_count(const uwie_mlp_trainer *trainer) { return trainer ? trainer->step : -1; }

int uwie_mlp_trainer_set_step_count(uwie_mlp_trainer *trainer, long long step)
{
    UWIE_REQUIRE(trainer != nullptr, "mlp_trainer_set_step_count: NULL trainer");
    UWIE_REQUIRE(step >= 0 && step < (1ll << 32), "mlp_trainer_set_step_count: step out of range (0 .. 2^32 - 1)");
    trainer->step = step;
    return UWIE_OK;
}

int uwie_mlp_trainer_eval(uwie_ctx *ctx, const uwie_mlp_trainer *trainer, const void *d_features, int features_are_f64, int batch,
                          float *d_out, void *d_workspace, size_t workspace_bytes, void *stream)
{
    UWIE_TRY(mlp_rows_check("mlp_trainer_eval", ctx, trainer, d_features, features_are_f64, batch, false, d_out, "d_out"));
    return mlp_eval(trainer->net, ctx, d_features, features_are_f64, batch, d_out, d_workspace, workspace_bytes, stream);
}

int uwie_u8_to_f32(uwie_ctx *ctx, const uint8_t *d_in, float *d_out, size_t n, void *stream)
{
    UWIE_REQUIRE(ctx && d_in && d_out, "u8_to_f32: NULL pointer");
    UWIE_REQUIRE(((uintptr_t)d_in & 3) == 0 && ((uintptr_t)d_out & 15) == 0, "u8_to_f32: d_in must be 4-byte, d_out 16-byte aligned");
    if (n == 0) return UWIE_OK;
    UWIE_SCOPE(ctx);
    return launch_u8_to_f32(d_in, n, d_out, (hipStream_t)stream);
}

int uwie_extract_features_u8(uwie_ctx *ctx, const uint8_t *d_in, float *d_features, int batch, int H, int W,
                             void *d_workspace, size_t workspace_bytes, void *stream)
{
    UWIE_REQUIRE(ctx && d_in && d_features, "extract_features: NULL pointer");
    UWIE_SCOPE(ctx);
    UWIE_CHECK_SHAPE(batch, H, W);
    const Shape s{batch, H, W};
    UWIE_CHECK_WS(features_ws_bytes(s));
    return launch_features_u8(d_in, s, d_features, d_workspace, (hipStream_t)stream);
}

int uwie_quality_scores(uwie_ctx *ctx, const uint8_t *d_u8, const float *d_f32, int batch, int H, int W, int gray_shift,
                        const double *weights8, double *d_scores, void *d_workspace, size_t workspace_bytes, void *stream)
{
    UWIE_REQUIRE(ctx && d_u8 && d_scores, "quality_scores: NULL pointer");
    UWIE_SCOPE(ctx);
    UWIE_CHECK_SHAPE(batch, H, W);
    UWIE_REQUIRE(gray_shift == 14 || gray_shift == 15, "gray_shift must be 14 or 15");
    static const double kDefault[8] = {0.20, 0.20, 0.15, 0.15, 0.10, 0.10, 0.05, 0.05};  // quality_assessment.py:229-238
    const Shape s{batch, H, W};
    UWIE_CHECK_WS(quality_ws_bytes(s));
    return launch_quality_scores(ctx, d_u8, d_f32, s, gray_shift, weights8 ? weights8 : kDefault, d_scores, d_workspace,
                                 (hipStream_t)stream);
}

size_t uwie_workspace_bytes_underwater(int batch, int H, int W)
{
    if (!shape_ok(batch, H, W) || batch > 65535) return 0;
    return underwater_ws_bytes(Shape{batch, H, W});
}

int uwie_underwater_plan(int H, int W, int *tile_w, int *tile_h)
{
    UWIE_REQUIRE(tile_w && tile_h, "underwater_plan: NULL pointer");
    UWIE_CHECK_SHAPE(1, H, W);
    underwater_tile(tile_w, tile_h);  // one tile for every frame
    return UWIE_OK;
}

int uwie_underwater_scores_u8(uwie_ctx *ctx, const uint8_t *d_u8, int batch, int H, int W, int gray_shift, double *d_scores,
                              void *d_workspace, size_t workspace_bytes, void *stream)
{
    UWIE_REQUIRE(ctx && d_u8 && d_scores, "underwater_scores: NULL pointer");
    UWIE_SCOPE(ctx);
    UWIE_CHECK_SHAPE(batch, H, W);
    UWIE_REQUIRE(batch <= 65535, "underwater_scores: batch must be <= 65535");
    UWIE_REQUIRE(gray_shift == 14 || gray_shift == 15, "gray_shift must be 14 or 15");
    const Shape s{batch, H, W};
    UWIE_CHECK_WS(underwater_ws_bytes(s));
    return launch_underwater_scores(ctx, d_u8, s, gray_shift, d_scores, d_workspace, (hipStream_t)stream);
}

size_t uwie_workspace_bytes_reference(int batch, int H, int W)
{
    if (!shape_ok(batch, H, W) || batch > 65535) return 0;
    return reference_ws_bytes(Shape{batch, H, W});
}

int uwie_reference_plan(int H, int W, int *tile_w, int *tile_h)
{
    UWIE_REQUIRE(tile_w && tile_h, "reference_plan: NULL pointer");
    UWIE_CHECK_SHAPE(1, H, W);
    reference_tile(tile_w, tile_h);  // one tile for every frame
    return UWIE_OK;
}

int uwie_reference_scores_u8(uwie_ctx *ctx, const uint8_t *d_u8, const uint8_t *d_ref_u8, int batch, int ref_batch, int H, int W,
                             int gray_shift, double *d_scores, void *d_workspace, size_t workspace_bytes, void *stream)
{
    UWIE_REQUIRE(ctx && d_u8 && d_ref_u8 && d_scores, "reference_scores: NULL pointer");
    UWIE_SCOPE(ctx);
    UWIE_CHECK_SHAPE(batch, H, W);
    UWIE_REQUIRE(batch <= 65535, "reference_scores: batch must be <= 65535");
    UWIE_REQUIRE(ref_batch >= 1 && ref_batch <= batch && batch % ref_batch == 0, "reference_scores: ref_batch must divide batch");
    UWIE_REQUIRE(gray_shift == 14 || gray_shift == 15, "gray_shift must be 14 or 15");
    const Shape s{batch, H, W};
    UWIE_CHECK_WS(reference_ws_bytes(s));
    return launch_reference_scores(d_u8, d_ref_u8, s, ref_batch, gray_shift, d_scores, d_workspace, (hipStream_t)stream);
}

size_t uwie_workspace_bytes_gray_world(int batch, int H, int W)
{
    if (!shape_ok(batch, H, W) || batch > 65535) return 0;
    return gray_world_ws_bytes(Shape{batch, H, W});
}

int uwie_gray_world_plan(int H, int W, int *block_px, int *thread_px)
{
    UWIE_REQUIRE(block_px && thread_px, "gray_world_plan: NULL pointer");
    UWIE_CHECK_SHAPE(1, H, W);
    gray_world_plan(block_px, thread_px);  // one pair for every frame
    return UWIE_OK;
}

int uwie_gray_world_u8(uwie_ctx *ctx, const uint8_t *d_in, int batch, int H, int W, double red, double blue, double max_gain,
                       uint8_t *d_out, double *d_stats, void *d_workspace, size_t workspace_bytes, void *stream)
{
    // every check comes before the context is touched
    UWIE_REQUIRE(ctx && d_in, "gray_world: NULL context or d_in");
    UWIE_REQUIRE(d_out || d_stats, "gray_world: d_out and d_stats are both NULL");
    UWIE_CHECK_SHAPE(batch, H, W);
    UWIE_REQUIRE(batch <= 65535, "gray_world: batch must be <= 65535");
    UWIE_REQUIRE(red >= 0.0 && red <= 1.0, "gray_world: red must be in [0, 1]");  // (false for NaN)
    UWIE_REQUIRE(blue >= 0.0 && blue <= 1.0, "gray_world: blue must be in [0, 1]");
    UWIE_REQUIRE(max_gain == 0.0 || (max_gain >= 1.0 && max_gain < HUGE_VAL), "gray_world: max_gain must be 0 (no bound) or finite and >= 1");
    UWIE_REQUIRE(((uintptr_t)d_in & 3) == 0 && ((uintptr_t)d_out & 3) == 0 && ((uintptr_t)d_stats & 7) == 0,
                 "gray_world: d_in and d_out must be 4-byte aligned, d_stats 8-byte aligned");
    const Shape s{batch, H, W};
    const size_t bytes = (size_t)batch * s.npx() * 3;
    UWIE_REQUIRE(!d_out || d_out == d_in || d_out + bytes <= d_in || d_in + bytes <= d_out,
                 "gray_world: d_out overlaps d_in partially (d_out == d_in is allowed)");
    UWIE_CHECK_WS(gray_world_ws_bytes(s));
    UWIE_SCOPE(ctx);
    return launch_gray_world(d_in, s, red, blue, max_gain, d_out, d_stats, d_workspace, (hipStream_t)stream);
}

size_t uwie_workspace_bytes_fusion(int batch, int H, int W, int levels)
{
    if (!shape_ok(batch, H, W) || batch > 65535 || levels < 1 || levels > 8) return 0;
    return fusion_ws_bytes(Shape{batch, H, W}, levels);
}

int uwie_fusion_plan(int H, int W, int levels, int *tile_w, int *tile_h)
{
    UWIE_REQUIRE(tile_w && tile_h, "fusion_plan: NULL pointer");
    UWIE_CHECK_SHAPE(1, H, W);
    UWIE_REQUIRE(levels >= 1 && levels <= 8, "fusion_plan: levels must be in 1 .. 8");
    fusion_tile(tile_w, tile_h);  // one tile for every frame and every levels
    return UWIE_OK;
}

int uwie_fusion_table(double gamma, uint8_t *table256)
{
    UWIE_REQUIRE(table256, "fusion_table: NULL table");
    UWIE_REQUIRE(gamma > 0.0 && gamma <= 8.0, "fusion_table: gamma must be finite, 0 < gamma <= 8");  // (false for NaN)
    fusion_table(gamma, table256);
    return UWIE_OK;
}

int uwie_fusion_u8(uwie_ctx *ctx, const uint8_t *d_in, int batch, int H, int W, double gamma, int levels, int gray_shift, uint8_t *d_out,
                   uint8_t *d_in1, uint8_t *d_in2, double *d_weight, void *d_workspace, size_t workspace_bytes, void *stream)
{
    // every check comes before the context is touched
    UWIE_REQUIRE(ctx && d_in && d_out, "fusion: NULL context, d_in or d_out");
    UWIE_CHECK_SHAPE(batch, H, W);
    UWIE_REQUIRE(batch <= 65535, "fusion: batch must be <= 65535");
    UWIE_REQUIRE(gamma > 0.0 && gamma <= 8.0, "fusion: gamma must be finite, 0 < gamma <= 8");  // (false for NaN)
    UWIE_REQUIRE(levels >= 1 && levels <= 8, "fusion: levels must be in 1 .. 8");
    UWIE_REQUIRE(gray_shift == 14 || gray_shift == 15, "fusion: gray_shift must be 14 or 15");
    UWIE_REQUIRE(((uintptr_t)d_weight & 7) == 0, "fusion: d_weight must be 8-byte aligned");
    const Shape s{batch, H, W};
    const size_t bytes = (size_t)batch * s.npx() * 3;
    const uint8_t *planes[4] = {d_in, d_out, d_in1, d_in2};  // d_out == d_in is the one overlap allowed
    for (int i = 0; i < 4; ++i)
        for (int j = i + 1; j < 4; ++j)
            UWIE_REQUIRE(!planes[i] || !planes[j] || (i == 0 && j == 1 && d_out == d_in) || planes[i] + bytes <= planes[j] ||
                             planes[j] + bytes <= planes[i],
                         "fusion: d_in, d_out, d_in1 and d_in2 overlap (only d_out == d_in is allowed)");
    UWIE_CHECK_WS(fusion_ws_bytes(s, levels));
    UWIE_SCOPE(ctx);
    return launch_fusion(d_in, s, gamma, levels, gray_shift, d_out, d_in1, d_in2, d_weight, d_workspace, (hipStream_t)stream);
}

int uwie_pick_best_u8(uwie_ctx *ctx, const double *d_scores, int n, int batch, int ncols, int col, const uint8_t *d_all_u8, int H,
                      int W, int32_t *d_best, uint8_t *d_best_u8, void *stream)
{
    UWIE_REQUIRE(ctx && d_scores && d_best, "pick_best: NULL pointer");
    UWIE_REQUIRE((d_all_u8 == nullptr) == (d_best_u8 == nullptr), "pick_best: d_all_u8 and d_best_u8 are given together");
    UWIE_SCOPE(ctx);
    UWIE_REQUIRE(n >= 1 && n <= 65535, "pick_best: 1 .. 65535 sets");
    UWIE_REQUIRE(ncols >= 1 && col >= 0 && col < ncols, "pick_best: column out of range");
    if (d_all_u8) {
        UWIE_CHECK_SHAPE(batch, H, W);
        UWIE_REQUIRE(batch <= 65535, "pick_best: batch must be <= 65535 to gather");
    } else {
        UWIE_REQUIRE(batch >= 1, "pick_best: batch must be >= 1");
        H = W = 1;
    }
    return launch_pick_best(d_scores, n, Shape{batch, H, W}, ncols, col, d_all_u8, d_best, d_best_u8, (hipStream_t)stream);
}

int uwie_feature_extractor_count(int H, int W)
{
    UWIE_REQUIRE(H >= 1 && W >= 1, "feature_extractor_count: H and W must be >= 1");
    return feature_extractor_count(H, W);
}

size_t uwie_workspace_bytes_feature_extractor(int batch, int H, int W)
{
    if (!shape_ok(batch, H, W) || batch > 65535) return 0;
    return feature_extractor_ws_bytes(Shape{batch, H, W});
}

int uwie_feature_extractor_u8(uwie_ctx *ctx, const uint8_t *d_u8, const float *d_f32, int batch, int H, int W, int gray_shift,
                              double *d_features, void *d_workspace, size_t workspace_bytes, void *stream)
{
    UWIE_REQUIRE(ctx && d_u8 && d_features, "feature_extractor: NULL pointer");
    UWIE_SCOPE(ctx);
    UWIE_CHECK_SHAPE(batch, H, W);
    UWIE_REQUIRE(batch <= 65535, "feature_extractor: batch must be <= 65535");
    UWIE_REQUIRE(gray_shift == 14 || gray_shift == 15, "gray_shift must be 14 or 15");
    const Shape s{batch, H, W};
    UWIE_CHECK_WS(feature_extractor_ws_bytes(s));
    return launch_feature_extractor(ctx, d_u8, d_f32, s, gray_shift, d_features, d_workspace, (hipStream_t)stream);
}

// ---------------------------------------------------------------- strategy classifier (k_classify.hip)
struct uwie_model : Handle<ClsModel> {};

int uwie_model_check(const uwie_model_desc *desc) { return classify_model_check(desc); }

int uwie_model_create(uwie_ctx *ctx, const uwie_model_desc *desc, uwie_model **out_model)
{
    UWIE_REQUIRE(ctx && out_model, "model_create: NULL context or out_model");
    *out_model = nullptr;
    UWIE_TRY(classify_model_check(desc));
    UWIE_SCOPE(ctx);
    const size_t bytes = classify_blob_bytes(desc);
    char *host = static_cast<char *>(calloc(bytes, 1));
    UWIE_REQUIRE(host != nullptr, "model_create: host allocation failed");
    void *blob = nullptr;
    hipError_t e = hipMalloc(&blob, bytes);
    ClsModel m{};
    if (e == hipSuccess) {
        m = classify_pack(desc, host, blob);
        e = hipMemcpy(blob, host, bytes, hipMemcpyHostToDevice);
    }
    free(host);
    if (e != hipSuccess) {
        if (blob) (void)hipFree(blob);
        set_error("model_create: upload of %zu bytes failed: %s", bytes, hipGetErrorString(e));
        return UWIE_E_HIP;
    }
    *out_model = new uwie_model{{ctx->device, m, blob}};
    return UWIE_OK;
}

void uwie_model_destroy(uwie_model *model) { handle_destroy(model); }

int uwie_model_info(const uwie_model *model, int *kind, int *n_classes, int *n_features)
{
    UWIE_REQUIRE(model != nullptr, "model_info: NULL model");
    if (kind) *kind = model->net.kind;
    if (n_classes) *n_classes = model->net.C;
    if (n_features) *n_features = model->net.F;
    return UWIE_OK;
}

int uwie_classify_f64(uwie_ctx *ctx, const uwie_model *model, const double *d_rows, int batch, int n_features, int32_t *d_label,
                      double *d_proba, void *stream)
{
    UWIE_REQUIRE(ctx && model && d_rows && d_label && d_proba, "classify: NULL pointer");
    UWIE_REQUIRE(model->device == ctx->device, "classify: the model lives on another device");
    UWIE_REQUIRE(batch >= 1 && batch <= (1 << 24), "classify: batch must be 1..2^24");
    if (n_features != model->net.F) {
        set_error("classify: rows have %d features, the model expects %d", n_features, model->net.F);
        return UWIE_E_INVALID;
    }
    UWIE_SCOPE(ctx);
    return launch_classify(model->net, d_rows, batch, d_label, d_proba, ctx->d_status, (hipStream_t)stream);
}

size_t uwie_workspace_bytes_predict(int batch, int H, int W)
{
    if (!shape_ok(batch, H, W) || batch > 65535) return 0;
    const Shape s{batch, H, W};
    Carver c(nullptr);
    c.take<double>((size_t)batch * feature_extractor_count(H, W));
    c.take<char>(feature_extractor_ws_bytes(s));
    return c.total();
}

int uwie_predict_strategy_u8(uwie_ctx *ctx, const uwie_model *model, const uint8_t *d_u8, const float *d_f32, int batch, int H,
                             int W, int gray_shift, int32_t *d_label, double *d_proba, double *d_rows, void *d_workspace,
                             size_t workspace_bytes, void *stream)
{
    UWIE_REQUIRE(ctx && model && d_u8 && d_label && d_proba, "predict: NULL pointer");
    UWIE_REQUIRE(model->device == ctx->device, "predict: the model lives on another device");
    UWIE_SCOPE(ctx);
    UWIE_CHECK_SHAPE(batch, H, W);
    UWIE_REQUIRE(batch <= 65535, "predict: batch must be <= 65535");
    UWIE_REQUIRE(gray_shift == 14 || gray_shift == 15, "gray_shift must be 14 or 15");
    const int n = feature_extractor_count(H, W);
    if (n != model->net.F) {
        set_error("predict: a %dx%d frame gives %d feature values, the model expects %d", H, W, n, model->net.F);
        return UWIE_E_INVALID;
    }
    const Shape s{batch, H, W};
    UWIE_CHECK_WS(uwie_workspace_bytes_predict(batch, H, W));
    Carver c(d_workspace);
    double *rows = c.take<double>((size_t)batch * n);
    void *fx_ws = c.take<char>(feature_extractor_ws_bytes(s));
    if (d_rows) rows = d_rows;
    hipStream_t st = (hipStream_t)stream;
    UWIE_TRY(launch_feature_extractor(ctx, d_u8, d_f32, s, gray_shift, rows, fx_ws, st));
    return launch_classify(model->net, rows, batch, d_label, d_proba, ctx->d_status, st);
}

int uwie_resize_rgb_u8(uwie_ctx *ctx, const uwie_frame_desc *d_desc, int batch, int out_h, int out_w, const uint8_t *d_flips,
                       uint8_t *d_out_u8, float *d_out_f32, float *d_out_norm, const float *mean3, const float *std3,
                       void *stream)
{
    UWIE_REQUIRE(ctx && d_desc, "resize_rgb: NULL pointer");
    UWIE_REQUIRE(d_out_u8 || d_out_f32 || d_out_norm, "resize_rgb: every output is NULL");
    UWIE_REQUIRE(!d_out_norm || (mean3 && std3), "resize_rgb: normalised output without mean / std");
    UWIE_REQUIRE(batch >= 1 && batch <= 65535, "resize_rgb: batch must be in [1, 65535]");
    UWIE_REQUIRE(out_h >= 1 && out_w >= 1 && out_h <= UWIE_RESIZE_MAX_SIDE && out_w <= UWIE_RESIZE_MAX_SIDE,
                 "resize_rgb: out_h / out_w must be in [1, UWIE_RESIZE_MAX_SIDE]");
    UWIE_SCOPE(ctx);
    return launch_resize_rgb(d_desc, batch, out_h, out_w, d_flips, d_out_u8, d_out_f32, d_out_norm, mean3, std3, ctx->d_status,
                             (hipStream_t)stream);
}

/* ---------------------------------------------------------------- stage entry points */

int uwie_cast_classify(uwie_ctx *ctx, const uint8_t *d_in, int batch, int H, int W, int32_t *d_kind, float *d_mean_rgb,
                       void *d_workspace, size_t workspace_bytes, void *stream)
{
    UWIE_REQUIRE(ctx && d_in && (d_kind || d_mean_rgb), "cast_classify: NULL pointer");
    UWIE_SCOPE(ctx);
    UWIE_CHECK_SHAPE(batch, H, W);
    const Shape s{batch, H, W};
    UWIE_CHECK_WS(cast_ws_bytes(s));
    return launch_cast_classify(ctx, d_in, s, d_kind, d_mean_rgb, d_workspace, (hipStream_t)stream);
}

int uwie_normalise_correct(uwie_ctx *ctx, const uint8_t *d_in, const int32_t *d_kind, float *d_out_f32, int batch, int H,
                           int W, void *stream)
{
    UWIE_REQUIRE(ctx && d_in && d_out_f32, "normalise_correct: NULL pointer");
    UWIE_SCOPE(ctx);
    UWIE_CHECK_SHAPE(batch, H, W);
    return launch_normalise_correct(d_in, d_kind, d_out_f32, Shape{batch, H, W}, (hipStream_t)stream);
}

int uwie_atmospheric_light(uwie_ctx *ctx, const uint8_t *d_in, const int32_t *d_kind, int batch, int H, int W,
                           const uwie_params *p, float *d_A, void *d_trace, void *d_workspace, size_t workspace_bytes,
                           void *stream)
{
    UWIE_REQUIRE(ctx && d_in && d_A && p, "atmospheric_light: NULL pointer");
    UWIE_SCOPE(ctx);
    UWIE_CHECK_SHAPE(batch, H, W);
    UWIE_REQUIRE(p->min_size >= 1 && (p->gray_shift == 14 || p->gray_shift == 15), "atmospheric_light: bad params");
    const Shape s{batch, H, W};
    Carver c(d_workspace);
    uint8_t *gray = c.take<uint8_t>((size_t)batch * s.npx());
    void *ws = c.take<char>(airlight_ws_bytes(s));
    UWIE_CHECK_WS(c.total());
    hipStream_t st = (hipStream_t)stream;
    return launch_airlight(ctx, d_in, d_kind, gray, s, p->min_size, d_A, d_trace, ws, st, p->gray_shift);
}

int uwie_transmission_init(uwie_ctx *ctx, const uint8_t *d_in, const int32_t *d_kind, const float *d_A, int batch, int H,
                           int W, const uwie_params *p, float *d_t0, uint8_t *d_gray, void *stream)
{
    UWIE_REQUIRE(ctx && d_in && d_A && p && (d_t0 || d_gray), "transmission_init: NULL pointer");
    UWIE_SCOPE(ctx);
    UWIE_CHECK_SHAPE(batch, H, W);
    const Shape s{batch, H, W};
    hipStream_t st = (hipStream_t)stream;
    const bool six = p->surface == UWIE_SURFACE_SIX;
    UWIE_REQUIRE(p->dark_patch >= 0 && p->dark_patch <= 31, "transmission_init: dark_patch must be 0 .. 31");
    if (d_t0)
        UWIE_TRY(launch_t0(FuseT0Args{d_in, d_kind, d_A, (float)p->omega, six ? 1e-6f : 1e-10f, six ? 1 : 0}, dark_patch_of(p), s, d_t0, st));
    if (d_gray) UWIE_TRY(launch_quant_gray(d_in, d_kind, d_gray, s, p->gray_shift, st));
    return UWIE_OK;
}

int uwie_box_filter_f64(uwie_ctx *ctx, const double *d_src, double *d_dst, int batch, int H, int W, int ksize,
                        void *d_workspace, size_t workspace_bytes, void *stream)
{
    UWIE_REQUIRE(ctx && d_src && d_dst, "box_filter: NULL pointer");
    UWIE_SCOPE(ctx);
    UWIE_CHECK_SHAPE(batch, H, W);
    UWIE_REQUIRE(ksize >= 1 && ksize <= 1024, "box_filter: ksize out of range");
    const Shape s{batch, H, W};
    UWIE_CHECK_WS(box_ws_bytes(s));
    return launch_box_filter_f64(d_src, d_dst, s, ksize, d_workspace, (hipStream_t)stream);
}

int uwie_guided_filter(uwie_ctx *ctx, const uint8_t *d_gray, const float *d_t0, int batch, int H, int W, int ksize,
                       double eps, int exact, double *d_t, void *d_workspace, size_t workspace_bytes, void *stream)
{
    UWIE_REQUIRE(ctx && d_gray && d_t0 && d_t, "guided_filter: NULL pointer");
    UWIE_SCOPE(ctx);
    UWIE_CHECK_SHAPE(batch, H, W);
    UWIE_REQUIRE(ksize >= 1 && ksize <= 1024, "guided_filter: ksize out of range");
    const Shape s{batch, H, W};
    UWIE_CHECK_WS(guided_ws_bytes(s));
    UWIE_REQUIRE(exact >= 0 && exact <= 2, "guided_filter: mode is 0 (fused float64), 1 (exact order) or 2 (fixed-point ring)");
    GuidedRequest r{ksize, eps, exact == 1};
    r.fx = exact == 2;
    return launch_guided_plan(plan_guided(s, r), s, d_gray, d_t0, d_t, d_workspace, (hipStream_t)stream);
}

int uwie_guided_plan(int batch, int H, int W, int ksize, int *split_row0, int *split_rows)
{
    UWIE_REQUIRE(split_row0 && split_rows, "guided_plan: NULL pointer");
    UWIE_CHECK_SHAPE(batch, H, W);
    const GuidedPlan g = plan_guided(Shape{batch, H, W}, {ksize, 1.0});  // (any eps > 0; the default tuning outside a context)
    const bool split = g.route == GF_SPLIT;
    *split_row0 = split ? g.iy0 : 0;
    *split_rows = split ? g.rows : 0;
    return UWIE_OK;
}

int uwie_guided_fill(int batch, int H, int W, int ksize, long long *items)
{
    UWIE_REQUIRE(items, "guided_fill: NULL pointer");
    UWIE_CHECK_SHAPE(batch, H, W);
    const Shape s{batch, H, W};
    const GuidedPlan g = plan_guided(s, {ksize, 1.0});
    *items = g.route == GF_SPLIT ? guided_items(s, g) : 0;
    return UWIE_OK;
}

int uwie_dark_patch_plan(int H, int W, int k, int *tile_w, int *tile_h)
{
    UWIE_REQUIRE(tile_w && tile_h, "dark_patch_plan: NULL pointer");
    UWIE_CHECK_SHAPE(1, H, W);
    UWIE_REQUIRE(k >= 0 && k <= 31, "dark_patch_plan: dark_patch must be 0 .. 31");
    dark_patch_tile(tile_w, tile_h);  // one tile for every patch and frame; k <= 1 launches k_trans_init, which has none
    return UWIE_OK;
}

int uwie_clahe_plan(int batch, int H, int W, int tiles_x, int tiles_y, double clip_limit, int recomputed,
                    uwie_clahe_plan_info *out)
{
    UWIE_REQUIRE(out, "clahe_plan: NULL pointer");
    UWIE_CHECK_SHAPE(batch, H, W);
    UWIE_REQUIRE(tiles_x >= 1 && tiles_y >= 1 && tiles_x * tiles_y <= 4096, "clahe_plan: bad tile grid");
    clahe_plan_info(Shape{batch, H, W}, clip_limit, tiles_x, tiles_y, recomputed != 0, out);
    return UWIE_OK;
}

int uwie_restore(uwie_ctx *ctx, const uint8_t *d_in, const int32_t *d_kind, const float *d_A, const double *d_t,
                 int batch, int H, int W, float *d_out_f32, void *stream)
{
    UWIE_REQUIRE(ctx && d_in && d_A && d_t && d_out_f32, "restore: NULL pointer");
    UWIE_SCOPE(ctx);
    UWIE_CHECK_SHAPE(batch, H, W);
    return launch_restore(d_in, d_kind, d_A, d_t, Shape{batch, H, W}, d_out_f32, (hipStream_t)stream);
}

int uwie_percentiles_f32(uwie_ctx *ctx, const float *d_img, int batch, int H, int W, const double *q_percent, int nq,
                         float *d_out, void *d_workspace, size_t workspace_bytes, void *stream)
{
    UWIE_REQUIRE(ctx && d_img && q_percent && d_out, "percentiles: NULL pointer");
    UWIE_SCOPE(ctx);
    UWIE_CHECK_SHAPE(batch, H, W);
    const Shape s{batch, H, W};
    UWIE_CHECK_WS(select_ws_bytes(s));
    return launch_percentiles(d_img, 0, s, q_percent, nq, d_out, d_workspace, (hipStream_t)stream);
}

int uwie_percentiles_f64(uwie_ctx *ctx, const double *d_img, int batch, int H, int W, const double *q_percent, int nq,
                         double *d_out, void *d_workspace, size_t workspace_bytes, void *stream)
{
    UWIE_REQUIRE(ctx && d_img && q_percent && d_out, "percentiles_f64: NULL pointer");
    UWIE_SCOPE(ctx);
    UWIE_CHECK_SHAPE(batch, H, W);
    const Shape s{batch, H, W};
    UWIE_CHECK_WS(select_ws_bytes(s));
    return launch_percentiles(d_img, 0, s, q_percent, nq, d_out, d_workspace, (hipStream_t)stream);
}

int uwie_enhance_percentiles(uwie_ctx *ctx, const void *d_workspace, size_t workspace_bytes, int batch, int H, int W,
                             const uwie_params *p, double *d_out, void *stream)
{
    UWIE_REQUIRE(ctx && d_workspace && d_out, "enhance_percentiles: NULL context, workspace or output pointer");
    UWIE_SCOPE(ctx);
    UWIE_CHECK_SHAPE(batch, H, W);
    UWIE_TRY(check_params(p));
    UWIE_REQUIRE(dehazes(p), "enhance_percentiles: only the dehazing strategies select percentiles in the workspace");
    const Shape s{batch, H, W};
    size_t need;
    const EnhanceLayout L = enhance_layout(const_cast<void *>(d_workspace), workspace_bytes, s, p, !ctx->last_enhance_f64, &need);
    UWIE_CHECK_WS(need);
    hipStream_t st = (hipStream_t)stream;
    const bool dict = p->surface == UWIE_SURFACE_DICT;
    const size_t per = (!dict && p->strategy == 3) ? 4 : 2;  // values per (image, channel)
    for (int i = 0; i < L.nsplit; ++i) {
        const size_t n = (size_t)L.cnt[i] * 3 * per;
        double *o = d_out + (size_t)L.start[i] * 3 * per;
        if (dict) UWIE_HIP_CHECK(hipMemcpyAsync(o, L.P[i].pct64, n * sizeof(double), hipMemcpyDeviceToDevice, st));
        else UWIE_TRY(launch_widen_f32(L.P[i].pct, o, n, st));
    }
    return UWIE_OK;
}

int uwie_stretch_f32(uwie_ctx *ctx, const float *d_img, float *d_out, int batch, int H, int W, double lo_percent,
                     double hi_percent, void *d_workspace, size_t workspace_bytes, void *stream)
{
    UWIE_REQUIRE(ctx && d_img && d_out, "stretch: NULL pointer");
    UWIE_SCOPE(ctx);
    UWIE_CHECK_SHAPE(batch, H, W);
    const Shape s{batch, H, W};
    Carver c(d_workspace);
    float *pct = c.take<float>((size_t)batch * 3 * 2);
    void *ws = c.take<char>(select_ws_bytes(s));
    UWIE_CHECK_WS(c.total());
    return stretch_f32(d_img, d_out, s, lo_percent, hi_percent, 1e-6f, pct, ws, (hipStream_t)stream);
}

int uwie_gamma_f32(uwie_ctx *ctx, const float *d_img, float *d_out, size_t n, double g, int mode, void *stream)
{
    UWIE_REQUIRE(ctx && d_img && d_out, "gamma: NULL pointer");
    UWIE_SCOPE(ctx);
    return launch_gamma_f32(d_img, d_out, n, g, mode, (hipStream_t)stream);
}

int uwie_clahe_f32(uwie_ctx *ctx, const float *d_img, float *d_out, int batch, int H, int W, double clip_limit,
                   int tiles_x, int tiles_y, void *d_workspace, size_t workspace_bytes, void *stream)
{
    UWIE_REQUIRE(ctx && d_img && d_out, "clahe: NULL pointer");
    UWIE_SCOPE(ctx);
    UWIE_CHECK_SHAPE(batch, H, W);
    UWIE_REQUIRE(tiles_x >= 1 && tiles_y >= 1 && tiles_x * tiles_y <= 4096, "clahe: bad tile grid");
    const Shape s{batch, H, W};
    UWIE_CHECK_WS(clahe_ws_bytes(s, tiles_x, tiles_y));
    return launch_clahe_f32(ctx, d_img, d_out, s, clip_limit, tiles_x, tiles_y, d_workspace, (hipStream_t)stream);
}

int uwie_rgb2gray_u8(uwie_ctx *ctx, const uint8_t *d_rgb, uint8_t *d_gray, size_t npixels, int gray_shift, void *stream)
{
    UWIE_REQUIRE(ctx && d_rgb && d_gray, "rgb2gray: NULL pointer");
    UWIE_SCOPE(ctx);
    UWIE_REQUIRE(gray_shift == 14 || gray_shift == 15, "gray_shift must be 14 or 15");
    return launch_rgb2gray_u8(d_rgb, d_gray, npixels, gray_shift, (hipStream_t)stream);
}

int uwie_rgb2lab_u8(uwie_ctx *ctx, const uint8_t *d_rgb, uint8_t *d_lab, size_t npixels, void *stream)
{
    UWIE_REQUIRE(ctx && d_rgb && d_lab, "rgb2lab: NULL pointer");
    UWIE_SCOPE(ctx);
    return launch_rgb2lab_u8(ctx, d_rgb, d_lab, npixels, (hipStream_t)stream);
}

int uwie_lab2rgb_u8(uwie_ctx *ctx, const uint8_t *d_lab, uint8_t *d_rgb, size_t npixels, void *stream)
{
    UWIE_REQUIRE(ctx && d_lab && d_rgb, "lab2rgb: NULL pointer");
    UWIE_SCOPE(ctx);
    return launch_lab2rgb_u8(ctx, d_lab, d_rgb, npixels, (hipStream_t)stream);
}

int uwie_clahe_u8(uwie_ctx *ctx, const uint8_t *d_plane, uint8_t *d_out, int batch, int H, int W, double clip_limit,
                  int tiles_x, int tiles_y, void *d_workspace, size_t workspace_bytes, void *stream)
{
    UWIE_REQUIRE(ctx && d_plane && d_out, "clahe_u8: NULL pointer");
    UWIE_SCOPE(ctx);
    UWIE_CHECK_SHAPE(batch, H, W);
    UWIE_REQUIRE(tiles_x >= 1 && tiles_y >= 1 && tiles_x * tiles_y <= 4096, "clahe: bad tile grid");
    const Shape s{batch, H, W};
    UWIE_CHECK_WS(clahe_ws_bytes(s, tiles_x, tiles_y));
    return launch_clahe_plane_u8(d_plane, d_out, s, clip_limit, tiles_x, tiles_y, d_workspace, (hipStream_t)stream);
}

int uwie_canny_u8(uwie_ctx *ctx, const uint8_t *d_gray, uint8_t *d_edges, int batch, int H, int W, int low, int high,
                  void *d_workspace, size_t workspace_bytes, void *stream)
{
    UWIE_REQUIRE(ctx && d_gray && d_edges, "canny: NULL pointer");
    UWIE_SCOPE(ctx);
    UWIE_CHECK_SHAPE(batch, H, W);
    if (low > high) { const int t = low; low = high; high = t; }
    const Shape s{batch, H, W};
    Carver c(d_workspace);
    Region *regs = c.take<Region>(batch);
    void *ws = c.take<char>(canny_ws_bytes(s));
    UWIE_CHECK_WS(c.total());
    hipStream_t st = (hipStream_t)stream;
    UWIE_TRY(launch_make_full_regions(regs, s, st));
    return launch_canny(d_gray, s, regs, batch, H, W, low, high, nullptr, d_edges, ws, st);
}

int uwie_equalize_hist_u8(uwie_ctx *ctx, const uint8_t *d_plane, uint8_t *d_out, int batch, int H, int W,
                          void *d_workspace, size_t workspace_bytes, void *stream)
{
    UWIE_REQUIRE(ctx && d_plane && d_out, "equalize_hist: NULL pointer");
    UWIE_SCOPE(ctx);
    UWIE_CHECK_SHAPE(batch, H, W);
    const Shape s{batch, H, W};
    UWIE_CHECK_WS((size_t)batch * 256 + 256);
    return launch_equalize_hist_u8(d_plane, d_out, s, d_workspace, (hipStream_t)stream);
}

}  // extern "C"
