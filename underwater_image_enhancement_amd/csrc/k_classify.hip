// The strategy classifier of main.py:398-433 (predict): StandardScaler.transform followed by a RandomForestClassifier,
// GradientBoostingClassifier or SVC(kernel='rbf', probability=True), one row per workgroup:
//   k_cls_trees<RF / GB>  the scaled row (float32, scikit-learn's DTYPE) sits in LDS, each lane walks whole trees and leaves
//                         the leaf's node index in LDS; then one lane per class sums the leaves in tree order (RF: class
//                         fractions; GB: learning_rate * value stage by stage), and lane 0 picks the label and the proba.
//   k_cls_svc             lanes over support vectors compute the RBF kernel values of a chunk into LDS, lanes over the
//                         one-vs-one pairs accumulate their decision values in libsvm's order across the chunks, and lane 0
//                         votes and runs the Platt sigmoid and multiclass_probability.
// A row's result depends only on that row: no atomics on results, no waits between workgroups, the same bits at every batch
// size.  The model was validated on the host (classify_model_check): every internal node's children lie strictly after it
// and inside its tree, so a walk ends within the tree's node count, and every feature index is in range.
#include <cmath>
#include <cstring>

#include "common.h"

namespace uwie {

namespace {

constexpr int kClsThreads = 256;
constexpr int kClsMaxF = 1024;     // uwie_model_check: n_features <= 1024
constexpr int kClsMaxC = 32;       // n_classes <= 32
constexpr int kClsMaxT = 4096;     // n_trees <= 4096
constexpr int kClsMaxNodes = 1 << 22;
constexpr int kClsMaxSV = 65536;
constexpr int kClsMaxP = kClsMaxC * (kClsMaxC - 1) / 2;
constexpr int kClsChunk = 1024;    // kernel values per LDS chunk (SVC)
constexpr int kClsPairsPerLane = (kClsMaxP + kClsThreads - 1) / kClsThreads;

// (x - mean) / scale, two float64 operations (StandardScaler.transform); any NaN raises the row's flag
__device__ __forceinline__ double cls_scaled(const ClsModel &m, const double *row, int f) { return (row[f] - m.mean[f]) / m.scale[f]; }

template <int KIND>
__global__ void __launch_bounds__(kClsThreads) k_cls_trees(ClsModel m, const double *__restrict__ rows, int32_t *__restrict__ label,
                                                           double *__restrict__ proba, uint32_t *__restrict__ status)
{
    __shared__ float s_x[kClsMaxF];
    __shared__ int s_leaf[kClsMaxT];
    __shared__ double s_acc[kClsMaxC];
    __shared__ int s_nan;
    const int b = blockIdx.x, tid = threadIdx.x;
    const double *row = rows + (size_t)b * m.F;
    if (tid == 0) s_nan = 0;
    __syncthreads();
    for (int f = tid; f < m.F; f += kClsThreads) {
        const double v = cls_scaled(m, row, f);
        s_x[f] = (float)v;
        if (v != v) s_nan = 1;
    }
    __syncthreads();
    if (KIND == UWIE_MODEL_GB && s_nan) {  // scikit-learn raises for the row: label -1, NaN proba, status bit
        for (int c = tid; c < m.C; c += kClsThreads) proba[(size_t)b * m.C + c] = __builtin_nan("");
        if (tid == 0) {
            label[b] = -1;
            atomicOr(status, (uint32_t)UWIE_STATUS_CLASSIFY_NAN);
        }
        return;
    }
    for (int t = tid; t < m.T; t += kClsThreads) {
        const int o = m.tree_off[t], cnt = m.tree_off[t + 1] - o;
        const ClsNode *nodes = m.nodes + o;
        int i = 0;
        for (int step = 0; step < cnt; ++step) {  // (children lie strictly after their parent: at most cnt steps)
            const ClsNode n = nodes[i];
            if (n.left < 0) break;
            const float x = s_x[n.feat];
            const bool go_left = (x != x) ? (n.miss != 0) : ((double)x <= n.thr);
            i = go_left ? n.left : n.right;
        }
        s_leaf[t] = o + i;
    }
    __syncthreads();
    if (KIND == UWIE_MODEL_RF) {
        // forest.predict_proba: ((0 + p_0) + p_1) + ... in tree order, then / n_estimators
        for (int c = tid; c < m.C; c += kClsThreads) {
            double acc = 0.0;
            for (int t = 0; t < m.T; ++t) acc += m.value[(size_t)s_leaf[t] * m.C + c];
            const double p = acc / (double)m.T;
            s_acc[c] = p;
            proba[(size_t)b * m.C + c] = p;
        }
        __syncthreads();
        if (tid == 0) {
            int best = 0;
            for (int c = 1; c < m.C; ++c)
                if (s_acc[c] > s_acc[best]) best = c;
            label[b] = best;
        }
    } else {
        // predict_stages: raw[k] = init[k], then raw[k] += learning_rate * value[leaf] stage by stage
        for (int k = tid; k < m.K; k += kClsThreads) {
            double raw = m.init[k];
            for (int t = k; t < m.T; t += m.K) raw += m.lr * m.value[s_leaf[t]];
            s_acc[k] = raw;
        }
        __syncthreads();
        if (tid == 0) {
            double *out = proba + (size_t)b * m.C;
            if (m.K == 1) {  // HalfBinomialLoss: expit, [1 - p, p]; label raw >= 0
                const double raw = s_acc[0];
                const double p = 1.0 / (1.0 + exp(-raw));
                out[0] = 1 - p;
                out[1] = p;
                label[b] = raw >= 0 ? 1 : 0;
            } else {  // HalfMultinomialLoss: softmax; label the first argmax of raw
                int best = 0;
                for (int k = 1; k < m.K; ++k)
                    if (s_acc[k] > s_acc[best]) best = k;
                const double mx = s_acc[best];
                double sum = 0.0;
                for (int k = 0; k < m.K; ++k) sum += exp(s_acc[k] - mx);
                for (int k = 0; k < m.K; ++k) out[k] = exp(s_acc[k] - mx) / sum;
                label[b] = best;
            }
        }
    }
}

// libsvm's sigmoid_predict
__device__ __forceinline__ double cls_sigmoid(double dec, double A, double B)
{
    const double fApB = dec * A + B;
    if (fApB >= 0) return exp(-fApB) / (1.0 + exp(-fApB));
    return 1.0 / (1 + exp(fApB));
}

__global__ void __launch_bounds__(kClsThreads) k_cls_svc(ClsModel m, const double *__restrict__ rows, int32_t *__restrict__ label,
                                                         double *__restrict__ proba, uint32_t *__restrict__ status)
{
    __shared__ double s_x[kClsMaxF];
    __shared__ double s_k[kClsChunk];
    __shared__ double s_dec[kClsMaxP];
    __shared__ double s_r[kClsMaxC * kClsMaxC];
    __shared__ double s_q[kClsMaxC * kClsMaxC];
    __shared__ double s_p[kClsMaxC], s_qp[kClsMaxC];
    __shared__ int s_vote[kClsMaxC];
    __shared__ int s_nan;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int C = m.C, P = C * (C - 1) / 2, S = m.S;
    const double *row = rows + (size_t)b * m.F;
    if (tid == 0) s_nan = 0;
    __syncthreads();
    for (int f = tid; f < m.F; f += kClsThreads) {
        const double v = cls_scaled(m, row, f);
        s_x[f] = v;
        if (v != v) s_nan = 1;
    }
    __syncthreads();
    if (s_nan) {
        for (int c = tid; c < C; c += kClsThreads) proba[(size_t)b * C + c] = __builtin_nan("");
        if (tid == 0) {
            label[b] = -1;
            atomicOr(status, (uint32_t)UWIE_STATUS_CLASSIFY_NAN);
        }
        return;
    }
    // this lane's pairs (i, j), i < j, in libsvm's order p = 0, 1, ...
    int pi[kClsPairsPerLane], pj[kClsPairsPerLane];
    double acc[kClsPairsPerLane];
#pragma unroll
    for (int u = 0; u < kClsPairsPerLane; ++u) {
        const int q = tid + u * kClsThreads;
        int i = 0, rem = q;
        while (i < C - 1 && rem >= C - 1 - i) rem -= C - 1 - i++;
        pi[u] = i;
        pj[u] = i + 1 + rem;
        acc[u] = 0.0;
    }
    for (int c0 = 0; c0 < S; c0 += kClsChunk) {
        const int n = min(kClsChunk, S - c0);
        for (int s = tid; s < n; s += kClsThreads) {
            const double *sv = m.svT + c0 + s;
            double d = 0.0;
            for (int f = 0; f < m.F; ++f) {
                const double diff = s_x[f] - sv[(size_t)f * S];
                d += diff * diff;
            }
            s_k[s] = exp(-m.gamma * d);
        }
        __syncthreads();
        // svm_predict_values: sum over class i's SVs with coef row j - 1, then class j's with row i; the classes' SVs are
        // contiguous and i's come first, so chunk after chunk keeps that order
#pragma unroll
        for (int u = 0; u < kClsPairsPerLane; ++u) {
            if (tid + u * kClsThreads >= P) break;
            const int i = pi[u], j = pj[u];
            const int ilo = max(m.sv_start[i], c0), ihi = min(m.sv_start[i + 1], c0 + n);
            const int jlo = max(m.sv_start[j], c0), jhi = min(m.sv_start[j + 1], c0 + n);
            const double *ci = m.coef + (size_t)(j - 1) * S, *cj = m.coef + (size_t)i * S;
            double a = acc[u];
            for (int s = ilo; s < ihi; ++s) a += ci[s] * s_k[s - c0];
            for (int s = jlo; s < jhi; ++s) a += cj[s] * s_k[s - c0];
            acc[u] = a;
        }
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < kClsPairsPerLane; ++u) {
        const int q = tid + u * kClsThreads;
        if (q < P) s_dec[q] = acc[u] - m.rho[q];
    }
    __syncthreads();
    if (tid != 0) return;
    // the one-vs-one vote (svm_predict_values); ties go to the lower class
    for (int c = 0; c < C; ++c) s_vote[c] = 0;
    for (int i = 0, q = 0; i < C; ++i)
        for (int j = i + 1; j < C; ++j, ++q) ++s_vote[s_dec[q] > 0 ? i : j];
    int best = 0;
    for (int c = 1; c < C; ++c)
        if (s_vote[c] > s_vote[best]) best = c;
    label[b] = best;
    // svm_predict_probability: pairwise Platt probabilities clamped to [1e-7, 1 - 1e-7], then multiclass_probability
    const double min_prob = 1e-7;
    for (int i = 0, q = 0; i < C; ++i)
        for (int j = i + 1; j < C; ++j, ++q) {
            const double v = fmin(fmax(cls_sigmoid(s_dec[q], m.prob_a[q], m.prob_b[q]), min_prob), 1 - min_prob);
            s_r[i * kClsMaxC + j] = v;
            s_r[j * kClsMaxC + i] = 1 - v;
        }
    double *Q = s_q, *p = s_p, *Qp = s_qp;
    const double *r = s_r;
    const int k = C;
    for (int t = 0; t < k; ++t) {
        p[t] = 1.0 / k;
        Q[t * kClsMaxC + t] = 0;
        for (int j = 0; j < t; ++j) {
            Q[t * kClsMaxC + t] += r[j * kClsMaxC + t] * r[j * kClsMaxC + t];
            Q[t * kClsMaxC + j] = Q[j * kClsMaxC + t];
        }
        for (int j = t + 1; j < k; ++j) {
            Q[t * kClsMaxC + t] += r[j * kClsMaxC + t] * r[j * kClsMaxC + t];
            Q[t * kClsMaxC + j] = -r[j * kClsMaxC + t] * r[t * kClsMaxC + j];
        }
    }
    const int max_iter = max(100, k);
    const double eps = 0.005 / k;
    for (int iter = 0; iter < max_iter; ++iter) {
        double pQp = 0;
        for (int t = 0; t < k; ++t) {
            Qp[t] = 0;
            for (int j = 0; j < k; ++j) Qp[t] += Q[t * kClsMaxC + j] * p[j];
            pQp += p[t] * Qp[t];
        }
        double max_error = 0;
        for (int t = 0; t < k; ++t) {
            const double error = fabs(Qp[t] - pQp);
            if (error > max_error) max_error = error;
        }
        if (max_error < eps) break;
        for (int t = 0; t < k; ++t) {
            const double diff = (-Qp[t] + pQp) / Q[t * kClsMaxC + t];
            p[t] += diff;
            pQp = (pQp + diff * (diff * Q[t * kClsMaxC + t] + 2 * Qp[t])) / (1 + diff) / (1 + diff);
            for (int j = 0; j < k; ++j) {
                Qp[j] = (Qp[j] + diff * Q[t * kClsMaxC + j]) / (1 + diff);
                p[j] /= (1 + diff);
            }
        }
    }
    for (int c = 0; c < C; ++c) proba[(size_t)b * C + c] = p[c];
}

bool finite_all(const double *a, size_t n)
{
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(a[i])) return false;
    return true;
}

size_t up256(size_t n) { return (n + 255) & ~size_t(255); }

// byte offsets of the blob's sections
struct BlobLayout {
    size_t mean, scale, tree_off, nodes, value, init, svT, coef, rho, prob_a, prob_b, sv_start, total;
};

BlobLayout blob_layout(const uwie_model_desc *d)
{
    BlobLayout L{};
    const size_t F = d->n_features, C = d->n_classes, P = C * (C - 1) / 2;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off = up256(off + bytes);
        return at;
    };
    L.mean = take(F * 8);
    L.scale = take(F * 8);
    if (d->kind == UWIE_MODEL_RF || d->kind == UWIE_MODEL_GB) {
        const size_t N = d->n_nodes, K = (d->kind == UWIE_MODEL_GB && C == 2) ? 1 : C;
        L.tree_off = take(((size_t)d->n_trees + 1) * 4);
        L.nodes = take(N * sizeof(ClsNode));
        L.value = take(N * (d->kind == UWIE_MODEL_RF ? C : 1) * 8);
        if (d->kind == UWIE_MODEL_GB) L.init = take(K * 8);
    } else {
        const size_t S = d->n_sv;
        L.svT = take(F * S * 8);
        L.coef = take((C - 1) * S * 8);
        L.rho = take(P * 8);
        L.prob_a = take(P * 8);
        L.prob_b = take(P * 8);
        L.sv_start = take((C + 1) * 4);
    }
    L.total = off;
    return L;
}

#define CLS_REQUIRE(cond, ...)               \
    do {                                     \
        if (!(cond)) {                       \
            set_error(__VA_ARGS__);          \
            return UWIE_E_INVALID;           \
        }                                    \
    } while (0)

}  // namespace

int classify_model_check(const uwie_model_desc *d)
{
    CLS_REQUIRE(d, "model_check: NULL descriptor");
    CLS_REQUIRE(d->kind == UWIE_MODEL_RF || d->kind == UWIE_MODEL_GB || d->kind == UWIE_MODEL_SVC, "model_check: unknown kind %d", d->kind);
    const int F = d->n_features, C = d->n_classes;
    CLS_REQUIRE(F >= 1 && F <= kClsMaxF, "model_check: n_features %d outside 1..%d", F, kClsMaxF);
    CLS_REQUIRE(C >= 2 && C <= kClsMaxC, "model_check: n_classes %d outside 2..%d", C, kClsMaxC);
    CLS_REQUIRE(d->mean && d->scale, "model_check: NULL mean or scale");
    CLS_REQUIRE(finite_all(d->mean, F) && finite_all(d->scale, F), "model_check: a non-finite mean or scale");
    for (int f = 0; f < F; ++f) CLS_REQUIRE(d->scale[f] != 0.0, "model_check: scale[%d] is zero", f);
    if (d->kind == UWIE_MODEL_SVC) {
        const int S = d->n_sv, P = C * (C - 1) / 2;
        CLS_REQUIRE(S >= 1 && S <= kClsMaxSV, "model_check: n_sv %d outside 1..%d", S, kClsMaxSV);
        CLS_REQUIRE(d->sv && d->dual_coef && d->intercept && d->n_support && d->prob_a && d->prob_b, "model_check: NULL SVC array");
        long long sum = 0;
        for (int c = 0; c < C; ++c) {
            CLS_REQUIRE(d->n_support[c] >= 0, "model_check: n_support[%d] is negative", c);
            sum += d->n_support[c];
        }
        CLS_REQUIRE(sum == S, "model_check: n_support sums to %lld, not n_sv %d", sum, S);
        CLS_REQUIRE(std::isfinite(d->gamma), "model_check: gamma is not finite");
        CLS_REQUIRE(finite_all(d->sv, (size_t)S * F) && finite_all(d->dual_coef, (size_t)(C - 1) * S) && finite_all(d->intercept, P) &&
                        finite_all(d->prob_a, P) && finite_all(d->prob_b, P),
                    "model_check: a non-finite support vector or coefficient");
        return UWIE_OK;
    }
    const int T = d->n_trees, N = d->n_nodes;
    CLS_REQUIRE(T >= 1 && T <= kClsMaxT, "model_check: n_trees %d outside 1..%d", T, kClsMaxT);
    CLS_REQUIRE(N >= 1 && N <= kClsMaxNodes, "model_check: n_nodes %d outside 1..%d", N, kClsMaxNodes);
    CLS_REQUIRE(d->tree_offset && d->left && d->right && d->feature && d->threshold && d->missing_left && d->value,
                "model_check: NULL tree array");
    CLS_REQUIRE(d->tree_offset[0] == 0 && d->tree_offset[T] == N, "model_check: tree offsets must run from 0 to n_nodes");
    for (int t = 0; t < T; ++t) {
        const int o = d->tree_offset[t], cnt = d->tree_offset[t + 1] - o;
        CLS_REQUIRE(cnt >= 1 && o + cnt <= N, "model_check: tree %d has no nodes or overruns n_nodes", t);
        for (int i = 0; i < cnt; ++i) {
            const int l = d->left[o + i], r = d->right[o + i];
            if (l == -1 && r == -1) continue;  // a leaf
            CLS_REQUIRE(l > i && l < cnt && r > i && r < cnt, "model_check: tree %d node %d has children %d, %d (need %d < child < %d)", t, i,
                        l, r, i, cnt);
            CLS_REQUIRE(d->feature[o + i] >= 0 && d->feature[o + i] < F, "model_check: tree %d node %d splits on feature %d of %d", t, i,
                        d->feature[o + i], F);
            CLS_REQUIRE(std::isfinite(d->threshold[o + i]), "model_check: tree %d node %d has a non-finite threshold", t, i);
        }
    }
    if (d->kind == UWIE_MODEL_RF) {
        CLS_REQUIRE(finite_all(d->value, (size_t)N * C), "model_check: a non-finite leaf value");
    } else {
        const int K = C == 2 ? 1 : C;
        CLS_REQUIRE(T % K == 0, "model_check: %d trees are not whole stages of %d", T, K);
        CLS_REQUIRE(d->init && finite_all(d->init, K), "model_check: NULL or non-finite init");
        CLS_REQUIRE(std::isfinite(d->learning_rate), "model_check: learning_rate is not finite");
        CLS_REQUIRE(finite_all(d->value, N), "model_check: a non-finite leaf value");
    }
    return UWIE_OK;
}

size_t classify_blob_bytes(const uwie_model_desc *d) { return blob_layout(d).total; }

// Lay a checked model out in host_blob (classify_blob_bytes bytes) and return its device view at dev_blob.
ClsModel classify_pack(const uwie_model_desc *d, void *host_blob, const void *dev_blob)
{
    const BlobLayout L = blob_layout(d);
    char *h = static_cast<char *>(host_blob);
    const char *g = static_cast<const char *>(dev_blob);
    const int F = d->n_features, C = d->n_classes;
    ClsModel m{};
    m.kind = d->kind;
    m.F = F;
    m.C = C;
    memcpy(h + L.mean, d->mean, (size_t)F * 8);
    memcpy(h + L.scale, d->scale, (size_t)F * 8);
    m.mean = reinterpret_cast<const double *>(g + L.mean);
    m.scale = reinterpret_cast<const double *>(g + L.scale);
    if (d->kind == UWIE_MODEL_SVC) {
        const int S = d->n_sv, P = C * (C - 1) / 2;
        m.S = S;
        m.gamma = d->gamma;
        double *svT = reinterpret_cast<double *>(h + L.svT);
        for (int s = 0; s < S; ++s)
            for (int f = 0; f < F; ++f) svT[(size_t)f * S + s] = d->sv[(size_t)s * F + f];
        memcpy(h + L.coef, d->dual_coef, (size_t)(C - 1) * S * 8);
        double *rho = reinterpret_cast<double *>(h + L.rho);
        for (int q = 0; q < P; ++q) rho[q] = -d->intercept[q];
        memcpy(h + L.prob_a, d->prob_a, (size_t)P * 8);
        memcpy(h + L.prob_b, d->prob_b, (size_t)P * 8);
        int32_t *start = reinterpret_cast<int32_t *>(h + L.sv_start);
        start[0] = 0;
        for (int c = 0; c < C; ++c) start[c + 1] = start[c] + d->n_support[c];
        m.svT = reinterpret_cast<const double *>(g + L.svT);
        m.coef = reinterpret_cast<const double *>(g + L.coef);
        m.rho = reinterpret_cast<const double *>(g + L.rho);
        m.prob_a = reinterpret_cast<const double *>(g + L.prob_a);
        m.prob_b = reinterpret_cast<const double *>(g + L.prob_b);
        m.sv_start = reinterpret_cast<const int32_t *>(g + L.sv_start);
        return m;
    }
    const int T = d->n_trees, N = d->n_nodes;
    m.T = T;
    m.K = (d->kind == UWIE_MODEL_GB && C == 2) ? 1 : C;
    memcpy(h + L.tree_off, d->tree_offset, ((size_t)T + 1) * 4);
    ClsNode *nodes = reinterpret_cast<ClsNode *>(h + L.nodes);
    for (int i = 0; i < N; ++i) {
        const bool leaf = d->left[i] == -1;
        nodes[i] = ClsNode{leaf ? 0.0 : d->threshold[i], d->left[i], d->right[i], leaf ? 0 : d->feature[i], d->missing_left[i] ? 1 : 0};
    }
    memcpy(h + L.value, d->value, (size_t)N * (d->kind == UWIE_MODEL_RF ? C : 1) * 8);
    m.tree_off = reinterpret_cast<const int32_t *>(g + L.tree_off);
    m.nodes = reinterpret_cast<const ClsNode *>(g + L.nodes);
    m.value = reinterpret_cast<const double *>(g + L.value);
    if (d->kind == UWIE_MODEL_GB) {
        m.lr = d->learning_rate;
        memcpy(h + L.init, d->init, (size_t)m.K * 8);
        m.init = reinterpret_cast<const double *>(g + L.init);
    }
    return m;
}

int launch_classify(const ClsModel &m, const double *d_rows, int B, int32_t *d_label, double *d_proba, uint32_t *d_status,
                    hipStream_t st)
{
    if (m.kind == UWIE_MODEL_RF) {
        UWIE_LAUNCH(k_cls_trees<UWIE_MODEL_RF>, dim3(B), dim3(kClsThreads), 0, st, m, d_rows, d_label, d_proba, d_status);
    } else if (m.kind == UWIE_MODEL_GB) {
        UWIE_LAUNCH(k_cls_trees<UWIE_MODEL_GB>, dim3(B), dim3(kClsThreads), 0, st, m, d_rows, d_label, d_proba, d_status);
    } else {
        UWIE_LAUNCH(k_cls_svc, dim3(B), dim3(kClsThreads), 0, st, m, d_rows, d_label, d_proba, d_status);
    }
    UWIE_LAUNCH_CHECK();
    return UWIE_OK;
}

}  // namespace uwie
