// Matching Networks head with a learned temperature (Vinyals et al. 2016): a query attends over the individual
// support rows of its episode in the cosine metric, and a class's score is the log of the attention mass that falls on it.  Per
// episode, with x^_i = x_i / max(|x_i|, eps), f^_q likewise, cos[q,i] = f^_q . x^_i and a = tau cos:
//     z[q,n] = logsumexp over the valid rows i of class n of a[q,i],   loss = mean over all B * Qn rows of logsumexp_n z[q,:] - z[q,y_q],
// which is the Matching Networks negative log-likelihood -log sum_{i: y_i = y_q} softmax_i(a[q,:]) written as a softmax cross-entropy of
// z: loss, correct, preds (first arg-max of z) and logits = z mean what they mean in every other head.  z is formed PER CLASS from the
// class's own maximum, never as the log of a sum of globally normalised probabilities: a class whose rows all lie far below the
// episode's best row keeps a finite, accurate logit.  The backward follows the same route: with dz = gs (softmax_n(z) - onehot(y_q)),
// gs = grad_scale / (B Qn), and r[q,i] the softmax of a within the class of row i,
//     da[q,i] = r[q,i] dz[q, y_i]      (= gs (p[q,i] - [y_i == y_q] r[q,i]) with p the softmax over all valid rows; rows of da sum to 0)
//     dtau = sum da cos,   dfeats_q = rq (G_q - f^_q (f^_q . G_q)),  G_q = tau sum_i da[q,i] x^_i,
//                          dfeats_s = rs (G_i - x^_i (x^_i . G_i)),  G_i = tau sum_q da[q,i] f^_q,
// rq, rs the reciprocal clamped norms; below the clamp the projection term is dropped (cosproto.hip's rule, and autograd's).  The
// normalised rows are never formed: both scales move into the epilogues of the products.
//
//   launch 1, one workgroup per (episode, 16 support rows): rs = 1 / max(|x_i|, eps) and whether |x_i| >= eps (16 lanes per row); the
//       first block of an episode also stages the labels, writes the class counts and reports the status bits.
//   launch 2, one workgroup per (episode, tile of 16 query rows): cos [16, S] = (f_tile X^T) rq rs on the f32 MFMA (wg_mm, 128 support
//       rows per call), kept in LDS; 16 lanes per row: the class maxima (one lane per class, rows in index order), e_i = exp(a_i -
//       max of its class), the class sums in index order, z = max + log(sum); then the rows kernels' softmax cross-entropy of z.  The
//       tile's loss / correct / dtau sums go to part[tile].  Training form: da = e_i dz[y_i] / sum[y_i] in place as tau da rs, and
//           dfeats_q = rq ((tau da rs) X - f_q rq tau sum_i da cos)              (wg_mm2, A read from LDS)
//       while tau da rq and tau da cos go to memory as [B, Qn, S] for launch 3.
//   launch 3, one workgroup per (episode, 16 support rows, 128 features), each over ALL Qn rows (no sum across workgroups):
//           dfeats_s = rs ((tau da rq)^T F_q - x_i rs sum_q tau da cos)          (the column sum in a fixed strided order)
//       and one further workgroup adds part[0..ntile): loss, correct, dtau.
//   The forward form (no gradient pointers) is launch 1, launch 2 without its backward half and the last workgroup of launch 3: the
//   same instructions produce loss, correct, preds and logits in both forms.
// Fixed summation orders, the first arg-max, the label-range rule and the absence of floating-point atomics are those of
// fewshot_head.h.  A support row left out takes no part and gets a zero gradient.  UNLIKE the prototype heads, a class without a valid
// support row has no zero prototype to fall back on: there is no row to attend to, so z = -inf for it (it carries no mass and is never
// predicted unless the whole row is NaN), FUMI_ST_CLASS_MISSING is set, and a query row labelled with it is left out exactly like a
// query label outside [0, N).  tau is read from device memory by the kernels.
#include "fewshot_head.h"

namespace {

constexpr float MH_EPS = 1e-12f;   // F.normalize's clamp
constexpr int MH_SMAX = 512;       // support rows of an episode: the [16, S] score image stays in LDS beside the product staging

__global__ __launch_bounds__(256) void match_prep_kernel(HeadDims d, int nsb, const float* __restrict__ xs,
                                                         const int64_t* __restrict__ ys, float* __restrict__ rsv,
                                                         float* __restrict__ sfl, int* __restrict__ cnt, int* status) {
    __shared__ int lab[MH_SMAX];
    const int tid = threadIdx.x;
    const int S = d.S, N = d.N, F = d.F;
    const int b = blockIdx.x / nsb, sb = blockIdx.x - b * nsb;
    const int row = tid >> 4, l = tid & 15, i = sb * FH_TM + row;
    {
        float s = 0.f;
        if (i < S) {
            const float* x = xs + ((long)b * S + i) * F;
            if ((((uintptr_t)x) & 15) == 0) {
                const f32x4* x4 = (const f32x4*)x;
                for (int k = l; k < (F >> 2); k += 16) { const f32x4 v = x4[k]; s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]; }
            } else {
                for (int k = l; k < F; k += 16) s += x[k] * x[k];
            }
        }
        for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (l == 0 && i < S) {
            const float nx = sqrtf(s);
            rsv[(long)b * S + i] = 1.f / fmaxf(nx, MH_EPS); sfl[(long)b * S + i] = nx >= MH_EPS ? 1.f : 0.f;
        }
    }
    if (sb != 0) return;
    if (fh_stage_labels(ys + (long)b * S, S, N, lab)) atomicOr(status, FUMI_ST_LABEL_RANGE);
    __syncthreads();
    if (tid < N) {
        const int c = fh_class_count(lab, S, tid);
        cnt[(long)b * N + tid] = c;
        if (c == 0) atomicOr(status, FUMI_ST_CLASS_MISSING);
    }
}

__global__ __launch_bounds__(256) void match_rows_kernel(HeadDims d, int lda, const float* __restrict__ xs, const int64_t* __restrict__ ys,
                                                         const float* __restrict__ fq, const int64_t* __restrict__ yq,
                                                         const float* __restrict__ rsv, const int* __restrict__ cnt,
                                                         const float* __restrict__ tau_p, int64_t* __restrict__ preds,
                                                         float* __restrict__ logits, float* __restrict__ part,
                                                         float* __restrict__ Wd, float* __restrict__ U, float* __restrict__ dfq,
                                                         int* status) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x;
    const int S = d.S, Qn = d.Qn, N = d.N, F = d.F;
    const int b = blockIdx.x / d.tpe, q0 = (blockIdx.x - b * d.tpe) * FH_TM, rows = min(FH_TM, Qn - q0);
    const long r0 = (long)b * Qn + q0;           // the tile's first row among all B * Qn
    float* Z = sm;                               // [16, lda] cos, then tau da rs
    float* rq = Z + FH_TM * lda;                 // [16] 1 / max(|f_q|, eps)
    float* se = rq + 16;                         // [16] |f_q| >= eps, then rq tau sum_i da cos where it is
    float* rl = se + 16;                         // [16] row losses, [16] row hits, [16] row dtau
    float* CM = rl + 48;                         // [16, 64] class maxima of a, then z
    float* GG = CM + FH_TM * 64;                 // [16, 64] dz_n / (class sum)
    float* RS = GG + FH_TM * 64;                 // [S] 1 / max(|x_i|, eps)
    int* lab = (int*)(RS + MH_SMAX);             // [S] labels, -1 where out of range
    float* mm = (float*)(lab + MH_SMAX);         // the products' staging; between them E [16, lda] = exp(a - class maximum)
    const float* ft = fq + r0 * F;
    const float* X = xs + (long)b * S * F;
    const float tau = tau_p[0];
    const int row = tid >> 4, l = tid & 15;      // 16 lanes per row
    const bool live = row < rows;

    (void)fh_stage_labels(ys + (long)b * S, S, N, lab);     // (launch 1 reported the labels out of range)
    for (int i = tid; i < S; i += 256) RS[i] = rsv[(long)b * S + i];
    for (int i = rows * lda + tid; i < FH_TM * lda; i += 256) Z[i] = 0.f;      // the rows past a ragged tile's end
    {
        float s = 0.f;
        if (live) {
            const float* x = ft + (long)row * F;
            if ((((uintptr_t)x) & 15) == 0) {
                const f32x4* x4 = (const f32x4*)x;
                for (int k = l; k < (F >> 2); k += 16) { const f32x4 v = x4[k]; s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]; }
            } else {
                for (int k = l; k < F; k += 16) s += x[k] * x[k];
            }
        }
        for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (l == 0) { const float nq = sqrtf(s); rq[row] = 1.f / fmaxf(nq, MH_EPS); se[row] = nq >= MH_EPS ? 1.f : 0.f; }
    }
    __syncthreads();
    for (int c0 = 0; c0 < S; c0 += FH_NB) {      // cos[m, c0 + n] = rq_m rs_n sum_f f[m, f] x[c0 + n, f]
        const int nb = min(FH_NB, S - c0);
        wg_mm(mm, FH_MM, rows, nb, F, ft, F, 1, X + (long)c0 * F, 1, F,
              [&](int m, int n, float acc) { Z[m * lda + c0 + n] = acc * rq[m] * RS[c0 + n]; });
    }
    __syncthreads();

    float* c = Z + row * lda;
    float* E = mm + row * lda;
    float* cmr = CM + row * 64;
    float* gr = GG + row * 64;
    // the class log-masses: lane l owns the classes l, l + 16, l + 32, l + 48 of its row and walks the support rows in index order
    float cm[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY}, cs[4] = {0.f, 0.f, 0.f, 0.f}, z[4];
    for (int i = 0; i < S; ++i) {
        const int lb = lab[i];
        const float a = tau * c[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) if (lb == l + 16 * j) cm[j] = fmaxf(cm[j], a);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) cmr[l + 16 * j] = cm[j];
    __syncthreads();
    for (int i = l; i < S; i += 16) { const int lb = lab[i]; E[i] = lb >= 0 ? expf(tau * c[i] - cmr[lb]) : 0.f; }
    __syncthreads();
    for (int i = 0; i < S; ++i) {
        const int lb = lab[i];
        const float e = E[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) if (lb == l + 16 * j) cs[j] += e;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) { z[j] = cm[j] + logf(cs[j]); cmr[l + 16 * j] = z[j]; }    // a class without a row: -inf + log(0) = -inf
    __syncthreads();

    {
        float loss = 0.f, hit = 0.f, dt = 0.f;
        // The row's softmax cross-entropy, the block of the four rows kernels (cosproto.hip) on z; it stays a copy as theirs do.
        float mx = -INFINITY; int arg = N;
#pragma unroll
        for (int j = 0; j < 4; ++j) { const int n = l + 16 * j; if (n < N && z[j] > mx) { mx = z[j]; arg = n; } }
        for (int o = 8; o > 0; o >>= 1) {
            const float v2 = __shfl_xor(mx, o, 64); const int a2 = __shfl_xor(arg, o, 64);
            if (v2 > mx || (v2 == mx && a2 < arg)) { mx = v2; arg = a2; }               // first arg-max (torch.max)
        }
        if (arg >= N) arg = 0;                                                           // (a row of NaNs, or no class with a row)
        float e[4], s = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) { e[j] = l + 16 * j < N ? expf(z[j] - mx) : 0.f; s += e[j]; }
        for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        long yv = live ? yq[r0 + row] : 0;
        const bool inr = yv >= 0 && yv < N;
        if (!inr) { if (l == 0) atomicOr(status, FUMI_ST_LABEL_RANGE); yv = 0; }
        const bool ok = live && inr && cnt[(long)b * N + yv] > 0;                        // a label of a class without a row: left out too
        loss = ok ? logf(s) - (cmr[yv] - mx) : 0.f;                                      // (the difference first: z is ~ tau + log count, the loss may be small)
        hit = (ok && arg == (int)yv) ? 1.f : 0.f;
        if (live) {
            if (l == 0 && preds) preds[r0 + row] = arg;
            if (logits) {
#pragma unroll
                for (int j = 0; j < 4; ++j) { const int n = l + 16 * j; if (n < N) logits[(r0 + row) * N + n] = z[j]; }
            }
        }
        if (d.train) {
            const float inv = 1.f / s;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int n = l + 16 * j;
                const float dz = ok ? d.gs * (e[j] * inv - (n == (int)yv ? 1.f : 0.f)) : 0.f;
                gr[n] = cs[j] > 0.f ? dz / cs[j] : 0.f;
            }
        }
        __syncthreads();
        if (d.train) {
            const float rqm = rq[row];
            float sd = 0.f;
            for (int i = l; i < S; i += 16) {
                const int lb = lab[i];
                const float cv = c[i];
                const float da = lb >= 0 ? E[i] * gr[lb] : 0.f;
                const float dc = tau * da;                                               // dcos
                dt += da * cv; sd += dc * cv;
                if (live) { Wd[(r0 + row) * S + i] = dc * rqm; U[(r0 + row) * S + i] = dc * cv; }
                c[i] = dc * RS[i];
            }
            for (int o = 8; o > 0; o >>= 1) { dt += __shfl_xor(dt, o, 64); sd += __shfl_xor(sd, o, 64); }
            if (l == 0) se[row] = se[row] * sd * rqm;
        }
        if (l == 0) { rl[row] = loss; rl[16 + row] = hit; rl[32 + row] = live ? dt : 0.f; }
    }
    __syncthreads();
    fh_tile_part<3>(rl, part, d.ntile);
    if (!d.train) return;
    // dfeats_tile [rows, F] = rq ((tau da rs) [rows, S] X [S, F] - f_tile se)
    for (int f0 = 0; f0 < F; f0 += FH_NB) {
        const int nb = min(FH_NB, F - f0);
        wg_mm2(mm, FH_MM, rows, nb, S, Z, lda, 1, X + f0, F, 1,
               [&](int m, int n) { return ft[(long)m * F + f0 + n]; },
               [&](int m, int n, float acc, float x) { dfq[(r0 + m) * F + f0 + n] = rq[m] * (acc - x * se[m]); });
    }
}

__global__ __launch_bounds__(256) void match_sgrad_kernel(HeadDims d, int nfb, int nsb, const float* __restrict__ xs,
                                                          const int64_t* __restrict__ ys, const float* __restrict__ fq,
                                                          const float* __restrict__ rsv, const float* __restrict__ sfl,
                                                          const float* __restrict__ Wd, const float* __restrict__ U,
                                                          const float* __restrict__ part, float* __restrict__ loss,
                                                          float* __restrict__ correct, float* __restrict__ dtau,
                                                          float* __restrict__ dfs) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x;
    const int S = d.S, Qn = d.Qn, N = d.N, F = d.F;
    if (blockIdx.x == gridDim.x - 1) {           // the sums over the row tiles
        fh_sum_parts<3>(part, d.ntile, sm, [&](const float (&t)[3]) {
            loss[0] = t[0] / (float)((long)d.B * Qn); correct[0] = t[1];
            if (dtau) dtau[0] = t[2];
        });
        return;
    }
    const int per = nsb * nfb;
    const int b = blockIdx.x / per, r = blockIdx.x - b * per, sb = r / nfb, fb = r - sb * nfb;
    const int i0 = sb * FH_TM, f0 = fb * FH_NB;
    const int ns = min(FH_TM, S - i0), nf = min(FH_NB, F - f0);
    float* ts = sm + FH_MM;                      // [16, 16] strided column sums of tau da cos
    float* rss = ts + 256;                       // [16] 1 / max(|x_i|, eps)
    float* tc = rss + 16;                        // [16] rs_i sum_q tau da cos where |x_i| >= eps, else 0
    float* vl = tc + 16;                         // [16] 1 where the row's label is in range
    {   // sum_q tau da[q, i] cos[q, i]: 16 strided partial sums per support row, added in index order
        const int c = tid & 15, j = tid >> 4;
        float s = 0.f;
        if (c < ns) {
            const float* u = U + (long)b * Qn * S + i0 + c;
#pragma unroll 4
            for (int k = j; k < Qn; k += 16) s += u[(long)k * S];
        }
        ts[j * 16 + c] = s;
        __syncthreads();
        if (j == 0 && c < ns) {
            float a = 0.f;
            for (int i = 0; i < 16; ++i) a += ts[i * 16 + c];
            const long t = ys[(long)b * S + i0 + c];
            const float rsi = rsv[(long)b * S + i0 + c];
            rss[c] = rsi; tc[c] = sfl[(long)b * S + i0 + c] != 0.f ? a * rsi : 0.f; vl[c] = (t >= 0 && t < N) ? 1.f : 0.f;
        }
    }
    __syncthreads();
    // dfeats_s[i0 + m, f0 + n] = rs_m (sum_k (tau da rq)[k, i0 + m] f_q[k, f0 + n] - x[i0 + m, f0 + n] tc_m); zero for a row left out
    wg_mm2(sm, FH_MM, ns, nf, Qn, Wd + (long)b * Qn * S + i0, 1, S, fq + (long)b * Qn * F + f0, F, 1,
           [&](int m, int n) { return xs[((long)b * S + i0 + m) * F + f0 + n]; },
           [&](int m, int n, float acc, float x) {
               dfs[((long)b * S + i0 + m) * F + f0 + n] = vl[m] != 0.f ? rss[m] * (acc - x * tc[m]) : 0.f;
           });
}

}  // namespace

extern "C" int fumi_hip_match_head_step(fumi_ws_t* ws, fumi_stream_t stream, int B, int S, int Qn, int N, int F,
        const float* feats_s, const int64_t* y_s, const float* feats_q, const int64_t* y_q, const float* tau, float grad_scale,
        float* loss, float* correct, int64_t* preds, float* logits, float* dfeats_s, float* dfeats_q, float* dtau) {
    if (int rc = head_args_check(ws, B, S, Qn, N, F, S <= MH_SMAX, {feats_s, y_s, feats_q, y_q, tau, loss, correct})) return rc;
    const int train = head_grad_form(dfeats_s, dfeats_q, dtau);
    if (train < 0) return FUMI_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(ws->device));
    const HeadDims d = head_dims_fill(B, S, Qn, N, F, train, grad_scale);
    const int lda = ((S + 15) & ~15) + 4;        // row stride of the score image
    const int nsb = (S + FH_TM - 1) / FH_TM, nfb = (F + FH_NB - 1) / FH_NB;
    const size_t n_rs = (size_t)B * S, n_cnt = (size_t)B * N, n_part = (size_t)3 * d.ntile, n_da = (size_t)B * Qn * S;
    int rc = ws_reserve(ws, 2 * ws_align(n_rs * 4) + ws_align(n_cnt * 4) + ws_align(n_part * 4) + (train ? 2 * ws_align(n_da * 4) : 0));
    if (rc) return rc;
    float* rsv = ws_f(ws, n_rs); float* sfl = ws_f(ws, n_rs); int* cnt = (int*)ws_f(ws, n_cnt); float* part = ws_f(ws, n_part);
    float* Wd = train ? ws_f(ws, n_da) : nullptr; float* U = train ? ws_f(ws, n_da) : nullptr;
    const size_t lds2 = ((size_t)FH_TM * lda + 80 + 2 * FH_TM * 64 + 2 * MH_SMAX + FH_MM) * 4;
    const size_t lds3 = train ? ((size_t)FH_MM + 256 + 48) * 4 : (size_t)768 * 4;   // the forward form's one workgroup only adds the tile sums
    hipLaunchKernelGGL(match_prep_kernel, dim3(B * nsb), dim3(256), 0, st, d, nsb, feats_s, y_s, rsv, sfl, cnt, ws->status);
    LAUNCH_CHECK();
    FUMI_SET_DYN_LDS(match_rows_kernel, lds2);
    hipLaunchKernelGGL(match_rows_kernel, dim3(d.ntile), dim3(256), lds2, st, d, lda, feats_s, y_s, feats_q, y_q, rsv, cnt, tau, preds,
                       logits, part, Wd, U, dfeats_q, ws->status);
    LAUNCH_CHECK();
    FUMI_SET_DYN_LDS(match_sgrad_kernel, lds3);
    hipLaunchKernelGGL(match_sgrad_kernel, dim3((train ? B * nsb * nfb : 0) + 1), dim3(256), lds3, st, d, nfb, nsb, feats_s, y_s, feats_q,
                       rsv, sfl, Wd, U, part, loss, correct, dtau, dfeats_s);
    LAUNCH_CHECK();
    return FUMI_OK;
}
