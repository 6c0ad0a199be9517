// Meta-step with the bf16 ResNet-12 image encoder at the im_net seam (fumi/models/fumi.py:89-100 is the seam; the inner loop, the
// query loss and the second-order outer gradient are fumi.py:146-192 / maml.py:156-191; BASELINE.json configs[4]).  Algorithm =
// oracle/resnet12_manual.py (forward-over-reverse second order, Pearlmutter), as conv4.hip does it for Conv4:
//
//   for t < T:   forward(theta_t) -> tape_t;  backward -> g_t;  theta_{t+1} = theta_t - alpha g_t          (support set)
//   query:       forward(theta_T) -> logits, loss;  backward -> bar_T
//   for t = T-1 .. 0:  bar_t = bar_{t+1} - alpha H_t bar_{t+1}   (one tangent forward + one tangent backward over tape_t)
//
// Memory plan.  HBM is the tape: every conv output, activation and gradient map of every inner step stays resident in bf16
// (12 maps per conv resolution and image: 4 u, 2 a, 4 du, 2 da, plus the pooled output and its gradient) -- 27 MB per 84 x 84 image
// and step at channels (64, 160, 320, 640), i.e. 13.6 GB for the 100 support images x 5 steps of a 20-way 5-shot episode, plus the
// query pass and one support-sized set of tangent maps.  288 GB hold a handful of such episodes, not a meta-batch of 64: the
// meta-batch is processed in CHUNKS of episodes (episodes are independent given the meta-parameters; the meta-gradient is the sum
// over chunks), the chunk size derived from the workspace budget.  Master weights and all parameter-space vectors are fp32.
#include "rn12.h"
#include "meta_front.h"
#include "conv4.h"                     // head kernels, axpy / broadcast / batched reduction (conv_ew.hip)
#include <string.h>
#include <stdlib.h>
#include <functional>

namespace {

struct RnLayer { int Cin, Cin_real, Cout, ntaps; long offW, offG, offB, fF, fB; };
struct RnNet {
    int B, nblk, Cimg, N, F;
    int C[RN_MAXBLK];
    RnGeom g[RN_MAXBLK + 1];                       // g[l]: conv resolution of block l; g[nblk]: the last pooled output
    RnLayer L[RN_MAXBLK][RN_NCONV];
    long PSZ, FSZ;                                 // per episode: floats of the parameter slab, bf16 elements of the fragment slab
};

int net_init(RnNet& n, int B, int nblk, int Cimg, int N, int H, int W, const int* channels) {
    if (nblk < 1 || nblk > RN_MAXBLK || Cimg < 1 || Cimg > 8 || B < 1 || N < 1 || !channels) return FUMI_EINVAL;
    n.B = B; n.nblk = nblk; n.Cimg = Cimg; n.N = N;
    long po = 0, fo = 0;
    int cin = 16, cin_real = Cimg;
    for (int l = 0; l < nblk; ++l) {
        const int c = channels[l];
        if (c < 32 || (c & 31) || c > 2048 || H < 2 || W < 2) return FUMI_EINVAL;
        n.C[l] = c; n.g[l] = rn_geom(H, W);
        if (rn_conv_lds_bytes(n.g[l], c) > 160 * 1024) return FUMI_ENOTSUP;
        for (int k = 0; k < RN_NCONV; ++k) {
            RnLayer& y = n.L[l][k];
            y.Cin = (k == 0 || k == 3) ? cin : c; y.Cin_real = (k == 0 || k == 3) ? cin_real : c;
            y.Cout = c; y.ntaps = k == 3 ? 1 : 9;
            y.offW = po; po += (long)c * y.Cin_real * y.ntaps;
            y.offG = po; po += c; y.offB = po; po += c;
            const long fe = (long)y.ntaps * y.Cin * c;
            y.fF = fo; fo += fe;
            const bool need_bwd = !(l == 0 && (k == 0 || k == 3));       // images are constants: no input gradient for block 1's c1 / cs
            y.fB = need_bwd ? fo : -1; if (need_bwd) fo += fe;
        }
        cin = c; cin_real = c; H /= 2; W /= 2;
    }
    n.g[nblk] = rn_geom(H, W);
    n.PSZ = (po + 63) / 64 * 64; n.FSZ = (fo + 127) / 128 * 128;
    n.F = channels[nblk - 1];
    return FUMI_OK;
}

struct RnPass {                                    // buffers of one pass over M images per episode
    int M;
    rbf16* u[RN_MAXBLK][4]; rbf16* a[RN_MAXBLK][2]; rbf16* out[RN_MAXBLK];
    rbf16* du[RN_MAXBLK][4]; rbf16* da[RN_MAXBLK][2]; rbf16* dout[RN_MAXBLK];
    float* coef[RN_MAXBLK][4];
    float* f; float* df; float* z; float* p; float* dz;
};
struct RnTan {                                     // tangent maps (support-sized, one inner step at a time)
    rbf16* ud[RN_MAXBLK][4]; rbf16* ad[RN_MAXBLK][2]; rbf16* outd[RN_MAXBLK];
    rbf16* dud[RN_MAXBLK][4]; rbf16* dad[RN_MAXBLK][2]; rbf16* doutd[RN_MAXBLK];
    float* fd; float* dfd; float* dzd;
};

size_t map_el(const RnNet& n, int M, int l) { return (size_t)n.B * M * n.g[l].Pp * n.C[l]; }
size_t out_el(const RnNet& n, int M, int l) { return (size_t)n.B * M * n.g[l + 1].Pp * n.C[l]; }
rbf16* ws_h(fumi_ws* ws, size_t n) { return (rbf16*)ws_f(ws, (n + 1) / 2); }

// the maps of a pass: `fwd` = what the forward writes and the backward reads (u, a, out, BN tables), `bwd` = what only the backward
// writes (du, da, dout).  A first-order tape keeps the forward part; the backward part can be shared by the passes of a lane.
size_t maps_bytes(const RnNet& n, int M, bool fwd, bool bwd) {
    size_t b = 0;
    for (int l = 0; l < n.nblk; ++l) {
        b += ((fwd ? 6 : 0) + (bwd ? 6 : 0)) * ws_align(map_el(n, M, l) * 2) + ((fwd ? 1 : 0) + (bwd ? 1 : 0)) * ws_align(out_el(n, M, l) * 2);
        if (fwd) b += 4 * ws_align((size_t)n.B * RCF_N * n.C[l] * 4);
    }
    return b;
}
void maps_carve(fumi_ws* ws, const RnNet& n, int M, bool fwd, bool bwd, RnPass& pb) {
    pb.M = M;
    for (int l = 0; l < n.nblk; ++l) {
        if (fwd) {
            for (int k = 0; k < 4; ++k) pb.u[l][k] = ws_h(ws, map_el(n, M, l));
            for (int k = 0; k < 2; ++k) pb.a[l][k] = ws_h(ws, map_el(n, M, l));
            pb.out[l] = ws_h(ws, out_el(n, M, l));
        }
        for (int k = 0; k < 4; ++k) pb.du[l][k] = bwd ? ws_h(ws, map_el(n, M, l)) : nullptr;
        for (int k = 0; k < 2; ++k) pb.da[l][k] = bwd ? ws_h(ws, map_el(n, M, l)) : nullptr;
        pb.dout[l] = bwd ? ws_h(ws, out_el(n, M, l)) : nullptr;
        if (fwd) for (int k = 0; k < 4; ++k) pb.coef[l][k] = ws_f(ws, (size_t)n.B * RCF_N * n.C[l]);
    }
}
size_t pass_bytes(const RnNet& n, int M, bool bwd) {
    return maps_bytes(n, M, true, bwd) + 2 * ws_align((size_t)n.B * M * n.F * 4) + 3 * ws_align((size_t)n.B * M * n.N * 4);
}
void pass_carve(fumi_ws* ws, const RnNet& n, int M, bool bwd, RnPass& pb) {
    maps_carve(ws, n, M, true, bwd, pb);
    pb.f = ws_f(ws, (size_t)n.B * M * n.F); pb.df = ws_f(ws, (size_t)n.B * M * n.F);
    pb.z = ws_f(ws, (size_t)n.B * M * n.N); pb.p = ws_f(ws, (size_t)n.B * M * n.N); pb.dz = ws_f(ws, (size_t)n.B * M * n.N);
}
size_t tan_bytes(const RnNet& n, int M) {
    size_t b = 0;
    for (int l = 0; l < n.nblk; ++l) b += 12 * ws_align(map_el(n, M, l) * 2) + 2 * ws_align(out_el(n, M, l) * 2);
    return b + 2 * ws_align((size_t)n.B * M * n.F * 4) + ws_align((size_t)n.B * M * n.N * 4);
}
void tan_carve(fumi_ws* ws, const RnNet& n, int M, RnTan& tb) {
    for (int l = 0; l < n.nblk; ++l) {
        for (int k = 0; k < 4; ++k) { tb.ud[l][k] = ws_h(ws, map_el(n, M, l)); tb.dud[l][k] = ws_h(ws, map_el(n, M, l)); }
        for (int k = 0; k < 2; ++k) { tb.ad[l][k] = ws_h(ws, map_el(n, M, l)); tb.dad[l][k] = ws_h(ws, map_el(n, M, l)); }
        tb.outd[l] = ws_h(ws, out_el(n, M, l)); tb.doutd[l] = ws_h(ws, out_el(n, M, l));
    }
    tb.fd = ws_f(ws, (size_t)n.B * M * n.F); tb.dfd = ws_f(ws, (size_t)n.B * M * n.F); tb.dzd = ws_f(ws, (size_t)n.B * M * n.N);
}

struct RnScratch { float* cpart; float* rpart; float* wpart; float* rowl; float* c2; size_t cpart_n, rpart_n, wpart_n, rowl_n, c2_n; };

size_t scratch_sizes(const RnNet& n, int S, int Qn, RnScratch& sc) {
    size_t cp = 0, rp = 0, wp = 0;
    const int Ms[2] = {S, Qn};
    for (int mi = 0; mi < 2; ++mi)
        for (int l = 0; l < n.nblk; ++l) {
            const long npix = (long)Ms[mi] * n.g[l].Pp;
            const size_t c1 = (size_t)n.B * rn_conv_tiles(npix, n.g[l]) * 2 * n.C[l];
            cp = c1 > cp ? c1 : cp;
            RnMap m; m.B = n.B; m.M = Ms[mi]; m.C = n.C[l]; m.g = n.g[l];
            const size_t r1 = (size_t)n.B * rn_red_nt(m) * 5 * n.C[l];
            rp = r1 > rp ? r1 : rp;
            for (int k = 0; k < RN_NCONV; ++k) {
                const RnLayer& y = n.L[l][k];
                const int Ci32 = (y.Cin + 31) / 32 * 32;
                const size_t w1 = (size_t)n.B * rn_wgrad_nsplit(n.B, npix, y.Cin, y.Cout) * y.ntaps * y.Cout * Ci32;
                wp = w1 > wp ? w1 : wp;
            }
        }
    sc.cpart_n = cp; sc.rpart_n = rp; sc.wpart_n = wp; sc.rowl_n = 2 * (size_t)n.B * (S > Qn ? S : Qn);
    sc.c2_n = (cp > rp ? cp : rp) / 32 + 4096;                       // first-stage sums of the coefficient kernel (groups of 64 slabs)
    return ws_align(cp * 4) + ws_align(rp * 4) + ws_align(wp * 4) + ws_align(sc.rowl_n * 4) + ws_align(sc.c2_n * 4);
}

#define TRY(expr) do { int _rc = (expr); if (_rc) return _rc; } while (0)
#define TRYP(phase, expr) do { ProfScope _ps(c.ws, c.st, phase); int _rc = (expr); if (_rc) return _rc; } while (0)

// `side` (the workspace's low-priority second stream, FUMI_RN_SIDE=0: off): the weight gradients are leaves of the backward chain
// (nothing in the pass reads them), MFMA-bound, and a quarter of the step, while a quarter of the chain itself is HBM-bound
// element-wise passes -- so they are forked off behind the map they read (ev[0]) and fill the matrix pipe under those passes;
// the pass joins (ev[1]) before it returns.  Their partial-sum scratch is touched by that stream only.  Measured: 568.8 -> 551.7 ms
// per 8-episode step (3 %: the convolutions and the weight gradients each hold 2 x 240 of a SIMD's 512 registers per lane, so the
// element-wise waves cannot sit beside them -- the gain is the tails of the launches filling up, not true co-residency).
// DropBlock / dropout on the pooled block outputs (the first-order encoder pair's _drop entries; off everywhere else): the rates,
// block sizes and seed as the caller passed them; set / b0 name the groups of the pass in flight (support 0 / query 1, the global
// index of the chunk's first episode)
struct RnDrop { bool on; float rate[RN_MAXBLK]; int block[RN_MAXBLK]; unsigned long long seed; int set, b0; };
struct RnCtx { fumi_ws* ws; hipStream_t st; RnNet n; RnScratch sc; hipStream_t side = nullptr; bool forked = false;
               hipEvent_t ev_fork = nullptr, ev_join = nullptr; RnDrop drop = {}; };

static hipStream_t rn_side_stream(fumi_ws* ws) {
    static const int on = getenv("FUMI_RN_SIDE") ? atoi(getenv("FUMI_RN_SIDE")) : 1;
    if (ws->profiling) return nullptr;              // phase timing (bench.py's roofline step): one stream, every phase on its own
    return on ? ws->side : nullptr;
}
// (a failed call may leave weight-gradient launches on the second stream: ws_abandon_lanes waits for it too)
// main waits for everything forked so far
static int rn_join(RnCtx& c) {
    if (!c.forked) return FUMI_OK;
    HIP_TRY(hipEventRecord(c.ev_join, c.side));
    HIP_TRY(hipStreamWaitEvent(c.st, c.ev_join, 0));
    c.forked = false;
    return FUMI_OK;
}

// bf16 fragment copies of one parameter slot (every layer, forward and backward-data order)
int frags_of_slot(hipStream_t st, const RnNet& n, const float* params, rbf16* frags) {
    for (int l = 0; l < n.nblk; ++l)
        for (int k = 0; k < RN_NCONV; ++k) {
            const RnLayer& y = n.L[l][k];
            TRY(launch_rn_wprep(st, n.B, y.Cout, y.Cin, y.Cin_real, y.ntaps, params + y.offW, n.PSZ, frags + y.fF,
                                y.fB >= 0 ? frags + y.fB : nullptr, n.FSZ));
        }
    return FUMI_OK;
}

RnMap map_of(const RnNet& n, int M, int l) { RnMap m; m.B = n.B; m.M = M; m.C = n.C[l]; m.g = n.g[l]; return m; }

RnSrc src_of(const rbf16* in, long in_stride, const rbf16* frag, long fstride, int Cin, int ntaps) {
    RnSrc s; s.in = in; s.in_stride = in_stride; s.frag = frag; s.frag_stride = fstride; s.Cin = Cin; s.ntaps = ntaps; return s;
}

// one conv (1..4 sources) + its statistics + the coefficient table of its BN
int conv_bn(RnCtx& c, int M, int l, int nsrc, const RnSrc* src, rbf16* out, const rbf16* dot, int mode, float* coef,
            const float* g, const float* beta, long pstride) {
    const RnNet& n = c.n;
    RnConvArgs a; memset(&a, 0, sizeof(a));
    a.B = n.B; a.nsrc = nsrc; a.Cout = n.C[l]; a.npix = (long)M * n.g[l].Pp; a.g = n.g[l];
    for (int s = 0; s < 4; ++s) a.src[s] = src[s < nsrc ? s : 0];
    a.out = out; a.out_stride = (long)M * n.g[l].Pp * n.C[l];
    a.stats = c.sc.cpart; a.dot = dot; a.dot_stride = a.out_stride;
    int nt = 0;
    TRYP(FUMI_PH_RN_CONV, launch_rn_conv(c.st, a, &nt));
    if ((size_t)n.B * nt * 2 * n.C[l] > c.sc.cpart_n) return FUMI_ENOMEM;        // (cannot happen: scratch_sizes bounds the tiles)
    RnCoefArgs ca; memset(&ca, 0, sizeof(ca));
    ca.B = n.B; ca.C = n.C[l]; ca.mode = mode; ca.nt = nt; ca.K = 2; ca.k0 = 0; ca.k1 = 1; ca.k2 = 0;
    ca.n = (float)((double)M * n.g[l].H * n.g[l].W);
    ca.part = c.sc.cpart; ca.coef = coef;
    if (mode == RCM_FWD) { ca.g = g; ca.beta = beta; ca.pstride = pstride; }
    else { ca.gd = g; ca.betad = beta; ca.dstride = pstride; }
    TRYP(FUMI_PH_RN_EW, launch_rn_coef(c.st, ca, c.sc.c2));
    return FUMI_OK;
}

// input-gradient convolution (no statistics)
int conv_plain(RnCtx& c, long npix, const RnGeom& g, int Cout, int nsrc, const RnSrc* src, rbf16* out) {
    RnConvArgs a; memset(&a, 0, sizeof(a));
    a.B = c.n.B; a.nsrc = nsrc; a.Cout = Cout; a.npix = npix; a.g = g;
    for (int s = 0; s < 4; ++s) a.src[s] = src[s < nsrc ? s : 0];
    a.out = out; a.out_stride = npix * Cout;
    TRYP(FUMI_PH_RN_CONV, launch_rn_conv(c.st, a));
    return FUMI_OK;
}

int wgrad(RnCtx& c, int M, int l, const RnLayer& y, int npair, const rbf16* x0, const rbf16* dy0, const rbf16* x1, const rbf16* dy1,
          float* G) {
    const RnNet& n = c.n;
    RnWgradArgs a; memset(&a, 0, sizeof(a));
    a.B = n.B; a.npair = npair; a.Cin = y.Cin; a.Cout = y.Cout; a.ntaps = y.ntaps; a.npix = (long)M * n.g[l].Pp; a.g = n.g[l];
    a.nsplit = rn_wgrad_nsplit(n.B, a.npix, y.Cin, y.Cout);
    a.x[0] = x0; a.dy[0] = dy0; a.x[1] = x1; a.dy[1] = dy1;
    a.x_stride = a.npix * y.Cin; a.dy_stride = a.npix * y.Cout;
    a.part = c.sc.wpart;
    hipStream_t st = c.st;
    if (c.side) {                                   // everything this product reads has been launched on the main stream by now
        HIP_TRY(hipEventRecord(c.ev_fork, c.st));
        HIP_TRY(hipStreamWaitEvent(c.side, c.ev_fork, 0));
        st = c.side; c.forked = true;
    }
    { ProfScope _ps(c.ws, st, FUMI_PH_RN_WGRAD); TRY(launch_rn_wgrad(st, a)); }
    { ProfScope _ps(c.ws, st, FUMI_PH_RN_WGRAD);
      TRY(launch_rn_wgrad_reduce(st, n.B, a.nsplit, y.ntaps, y.Cout, y.Cin, y.Cin_real, c.sc.wpart, G + y.offW, n.PSZ)); }
    return FUMI_OK;
}

RnJoin join_of(const RnNet& n, int M, int l, const RnPass& pb, const RnTan* tb) {
    RnJoin j; memset(&j, 0, sizeof(j));
    j.m = map_of(n, M, l); j.gn = n.g[l + 1]; j.Ho = n.g[l].H / 2; j.Wo = n.g[l].W / 2;
    j.u3 = pb.u[l][2]; j.us = pb.u[l][3]; j.coef3 = pb.coef[l][2]; j.coefs = pb.coef[l][3];
    if (tb) { j.u3d = tb->ud[l][2]; j.usd = tb->ud[l][3]; }
    return j;
}

// map <- keep * scale * map for block l's pooled output (forward) or its adjoint (backward): a count launch, then the apply launch.
// The counters sit at the head of the backward's reduction scratch, idle at both places (the forward never uses it; in the backward
// the join's reduction, next on this stream, overwrites it).  Blocks with rate 0 launch nothing.
int drop_map(RnCtx& c, int M, int l, rbf16* map) {
    const RnDrop& d = c.drop;
    if (!d.on || !(d.rate[l] > 0.f)) return FUMI_OK;
    const RnNet& n = c.n;
    if ((size_t)4 * n.B > c.sc.rpart_n) return FUMI_ENOMEM;                      // (cannot happen: 5 C floats per episode and slab)
    unsigned long long* kept = (unsigned long long*)c.sc.rpart;
    TRYP(FUMI_PH_RN_EW, launch_rn_drop(c.st, n.B, M, n.g[l + 1], n.C[l], d.rate[l], d.block[l], d.seed, l, d.set, d.b0, map, kept,
                                       (unsigned*)(kept + n.B), c.sc.rpart + 3 * (size_t)n.B, true, true));
    return FUMI_OK;
}

int forward_pass(RnCtx& c, int M, const rbf16* img16, const float* params, const rbf16* frags, RnPass& pb, const float* head,
                 const int64_t* y, float scale, float* logits, int64_t* preds, float* preds_f, float* loss_b, float* acc_b) {
    const RnNet& n = c.n;
    for (int l = 0; l < n.nblk; ++l) {
        const RnLayer* L = n.L[l];
        const rbf16* xin = l ? pb.out[l - 1] : img16;
        const long xs = (long)M * n.g[l].Pp * L[0].Cin, ms = (long)M * n.g[l].Pp * n.C[l];
        const RnMap m = map_of(n, M, l);
        RnSrc s[4];
        s[0] = src_of(xin, xs, frags + L[0].fF, n.FSZ, L[0].Cin, 9);
        TRY(conv_bn(c, M, l, 1, s, pb.u[l][0], nullptr, RCM_FWD, pb.coef[l][0], params + L[0].offG, params + L[0].offB, n.PSZ));
        TRYP(FUMI_PH_RN_EW, launch_rn_act(c.st, m, pb.u[l][0], nullptr, pb.coef[l][0], pb.a[l][0]));
        s[0] = src_of(pb.a[l][0], ms, frags + L[1].fF, n.FSZ, L[1].Cin, 9);
        TRY(conv_bn(c, M, l, 1, s, pb.u[l][1], nullptr, RCM_FWD, pb.coef[l][1], params + L[1].offG, params + L[1].offB, n.PSZ));
        TRYP(FUMI_PH_RN_EW, launch_rn_act(c.st, m, pb.u[l][1], nullptr, pb.coef[l][1], pb.a[l][1]));
        s[0] = src_of(pb.a[l][1], ms, frags + L[2].fF, n.FSZ, L[2].Cin, 9);
        TRY(conv_bn(c, M, l, 1, s, pb.u[l][2], nullptr, RCM_FWD, pb.coef[l][2], params + L[2].offG, params + L[2].offB, n.PSZ));
        s[0] = src_of(xin, xs, frags + L[3].fF, n.FSZ, L[3].Cin, 1);
        TRY(conv_bn(c, M, l, 1, s, pb.u[l][3], nullptr, RCM_FWD, pb.coef[l][3], params + L[3].offG, params + L[3].offB, n.PSZ));
        TRYP(FUMI_PH_RN_EW, launch_rn_join_fwd(c.st, join_of(n, M, l, pb, nullptr), pb.out[l], 0));
        TRY(drop_map(c, M, l, pb.out[l]));
    }
    TRYP(FUMI_PH_RN_EW, launch_rn_avgpool(c.st, n.B * M, n.F, n.g[n.nblk], pb.out[n.nblk - 1], pb.f));
    if (!head) return FUMI_OK;
    HeadArgs h; memset(&h, 0, sizeof(h));
    h.B = n.B; h.M = M; h.N = n.N; h.F = n.F; h.scale = scale; h.f = pb.f; h.head = head; h.y = y;
    h.z = logits ? logits : pb.z; h.p = pb.p; h.dz = pb.dz; h.preds = preds; h.preds_f = preds_f; h.loss_b = loss_b; h.acc_b = acc_b;
    h.status = c.ws->status; h.row_loss = c.sc.rowl; h.row_hit = c.sc.rowl + (size_t)n.B * M;
    TRYP(FUMI_PH_RN_EW, launch_head_logits(c.st, h));
    return FUMI_OK;
}

// BWD coefficients of one BN from reduced partial sums (slices k0 / k1 of K) + its weight / bias gradients
int coef_bwd(RnCtx& c, int M, int l, int nt, int K, int k0, int k1, int k2, int mode, float* coef, const float* gd, float* dg, float* db) {
    const RnNet& n = c.n;
    RnCoefArgs ca; memset(&ca, 0, sizeof(ca));
    ca.B = n.B; ca.C = n.C[l]; ca.mode = mode; ca.nt = nt; ca.K = K; ca.k0 = k0; ca.k1 = k1; ca.k2 = k2;
    ca.n = (float)((double)M * n.g[l].H * n.g[l].W);
    ca.part = c.sc.rpart; ca.coef = coef; ca.gd = gd; ca.dstride = n.PSZ; ca.dg = dg; ca.dbeta = db; ca.gstride = n.PSZ;
    TRYP(FUMI_PH_RN_EW, launch_rn_coef(c.st, ca, c.sc.c2));
    return FUMI_OK;
}

// G [B][PSZ], dh [B][N][F+1]: gradient of the pass's loss (head == NULL: the feature adjoints are already in pb.df)
int backward_pass(RnCtx& c, int M, const rbf16* img16, const rbf16* frags, RnPass& pb, const float* head, float* G, float* dh) {
    const RnNet& n = c.n;
    if (head) {
        HeadGradArgs hg; memset(&hg, 0, sizeof(hg));
        hg.B = n.B; hg.M = M; hg.N = n.N; hg.F = n.F; hg.nsrc = 1; hg.dz[0] = pb.dz; hg.f[0] = pb.f; hg.head[0] = head;
        hg.dh = dh; hg.df = pb.df;
        TRYP(FUMI_PH_RN_EW, launch_head_grad(c.st, hg));
    }
    TRYP(FUMI_PH_RN_EW, launch_rn_avgpool_bwd(c.st, n.B * M, n.F, n.g[n.nblk], pb.df, pb.dout[n.nblk - 1]));
    for (int l = n.nblk - 1; l >= 0; --l) {
        const RnLayer* L = n.L[l];
        const rbf16* xin = l ? pb.out[l - 1] : img16;
        const long npix = (long)M * n.g[l].Pp, ms = npix * n.C[l];
        const RnMap m = map_of(n, M, l);
        const int nt = rn_red_nt(m);
        const RnJoin j = join_of(n, M, l, pb, nullptr);
        TRY(drop_map(c, M, l, pb.dout[l]));                // (the join's backward reads u3 / us and dout, never out[l])
        TRYP(FUMI_PH_RN_EW, launch_rn_join_reduce(c.st, j, pb.dout[l], nullptr, c.sc.rpart, 0));
        TRY(coef_bwd(c, M, l, nt, 3, 0, 1, 0, RCM_BWD, pb.coef[l][2], nullptr, G + L[2].offG, G + L[2].offB));
        TRY(coef_bwd(c, M, l, nt, 3, 0, 2, 0, RCM_BWD, pb.coef[l][3], nullptr, G + L[3].offG, G + L[3].offB));
        TRYP(FUMI_PH_RN_EW, launch_rn_join_apply(c.st, j, pb.dout[l], nullptr, pb.du[l][2], pb.du[l][3], 0));
        RnSrc s[4];
        for (int k = 2; k >= 1; --k) {                    // c3 then c2: weight gradient, input gradient, the BN below
            TRY(wgrad(c, M, l, L[k], 1, pb.a[l][k - 1], pb.du[l][k], nullptr, nullptr, G));
            s[0] = src_of(pb.du[l][k], ms, frags + L[k].fB, n.FSZ, n.C[l], 9);
            TRY(conv_plain(c, npix, n.g[l], n.C[l], 1, s, pb.da[l][k - 1]));
            TRYP(FUMI_PH_RN_EW, launch_rn_bwd_reduce(c.st, m, pb.u[l][k - 1], nullptr, pb.da[l][k - 1], nullptr, pb.coef[l][k - 1], c.sc.rpart, 0));
            TRY(coef_bwd(c, M, l, nt, 2, 0, 1, 0, RCM_BWD, pb.coef[l][k - 1], nullptr, G + L[k - 1].offG, G + L[k - 1].offB));
            TRYP(FUMI_PH_RN_EW, launch_rn_bwd_apply(c.st, m, pb.u[l][k - 1], nullptr, pb.da[l][k - 1], nullptr, pb.coef[l][k - 1], pb.du[l][k - 1], 0));
        }
        TRY(wgrad(c, M, l, L[0], 1, xin, pb.du[l][0], nullptr, nullptr, G));
        TRY(wgrad(c, M, l, L[3], 1, xin, pb.du[l][3], nullptr, nullptr, G));
        if (l) {
            s[0] = src_of(pb.du[l][0], ms, frags + L[0].fB, n.FSZ, n.C[l], 9);
            s[1] = src_of(pb.du[l][3], ms, frags + L[3].fB, n.FSZ, n.C[l], 1);
            TRY(conv_plain(c, npix, n.g[l], n.C[l - 1], 2, s, pb.dout[l - 1]));
        }
    }
    return rn_join(c);
}

// HV [B][PSZ], HVh [B][N][F+1] = Hessian of the support loss at the tape's parameters times (V, Vh)
int hvp_pass(RnCtx& c, int M, const rbf16* img16, const rbf16* frags, RnPass& pb, RnTan& tb, const float* head, const float* V,
             const rbf16* Vfrags, const float* Vh, float scale, float* HV, float* HVh) {
    const RnNet& n = c.n;
    // ---- tangent forward
    for (int l = 0; l < n.nblk; ++l) {
        const RnLayer* L = n.L[l];
        const rbf16* xin = l ? pb.out[l - 1] : img16;
        const rbf16* xind = l ? tb.outd[l - 1] : nullptr;
        const long xs = (long)M * n.g[l].Pp * L[0].Cin, ms = (long)M * n.g[l].Pp * n.C[l];
        const RnMap m = map_of(n, M, l);
        RnSrc s[4];
        s[0] = src_of(xin, xs, Vfrags + L[0].fF, n.FSZ, L[0].Cin, 9);
        if (xind) s[1] = src_of(xind, xs, frags + L[0].fF, n.FSZ, L[0].Cin, 9);
        TRY(conv_bn(c, M, l, xind ? 2 : 1, s, tb.ud[l][0], pb.u[l][0], RCM_TFWD, pb.coef[l][0], V + L[0].offG, V + L[0].offB, n.PSZ));
        TRYP(FUMI_PH_RN_EW, launch_rn_act(c.st, m, pb.u[l][0], tb.ud[l][0], pb.coef[l][0], tb.ad[l][0]));
        for (int k = 1; k <= 2; ++k) {
            s[0] = src_of(pb.a[l][k - 1], ms, Vfrags + L[k].fF, n.FSZ, n.C[l], 9);
            s[1] = src_of(tb.ad[l][k - 1], ms, frags + L[k].fF, n.FSZ, n.C[l], 9);
            TRY(conv_bn(c, M, l, 2, s, tb.ud[l][k], pb.u[l][k], RCM_TFWD, pb.coef[l][k], V + L[k].offG, V + L[k].offB, n.PSZ));
            if (k == 1) TRYP(FUMI_PH_RN_EW, launch_rn_act(c.st, m, pb.u[l][1], tb.ud[l][1], pb.coef[l][1], tb.ad[l][1]));
        }
        s[0] = src_of(xin, xs, Vfrags + L[3].fF, n.FSZ, L[3].Cin, 1);
        if (xind) s[1] = src_of(xind, xs, frags + L[3].fF, n.FSZ, L[3].Cin, 1);
        TRY(conv_bn(c, M, l, xind ? 2 : 1, s, tb.ud[l][3], pb.u[l][3], RCM_TFWD, pb.coef[l][3], V + L[3].offG, V + L[3].offB, n.PSZ));
        TRYP(FUMI_PH_RN_EW, launch_rn_join_fwd(c.st, join_of(n, M, l, pb, &tb), tb.outd[l], 1));
    }
    TRYP(FUMI_PH_RN_EW, launch_rn_avgpool(c.st, n.B * M, n.F, n.g[n.nblk], tb.outd[n.nblk - 1], tb.fd));
    HeadArgs h; memset(&h, 0, sizeof(h));
    h.B = n.B; h.M = M; h.N = n.N; h.F = n.F; h.scale = scale; h.f = pb.f; h.head = head; h.y = nullptr;
    h.fd = tb.fd; h.headd = Vh; h.p = pb.p; h.dz = tb.dzd;
    TRYP(FUMI_PH_RN_EW, launch_head_logits(c.st, h));
    // ---- tangent backward
    HeadGradArgs hg; memset(&hg, 0, sizeof(hg));
    hg.B = n.B; hg.M = M; hg.N = n.N; hg.F = n.F; hg.nsrc = 2;
    hg.dz[0] = tb.dzd; hg.f[0] = pb.f; hg.head[0] = head;
    hg.dz[1] = pb.dz; hg.f[1] = tb.fd; hg.head[1] = Vh;
    hg.dh = HVh; hg.df = tb.dfd;
    TRYP(FUMI_PH_RN_EW, launch_head_grad(c.st, hg));
    TRYP(FUMI_PH_RN_EW, launch_rn_avgpool_bwd(c.st, n.B * M, n.F, n.g[n.nblk], tb.dfd, tb.doutd[n.nblk - 1]));
    for (int l = n.nblk - 1; l >= 0; --l) {
        const RnLayer* L = n.L[l];
        const rbf16* xin = l ? pb.out[l - 1] : img16;
        const rbf16* xind = l ? tb.outd[l - 1] : nullptr;
        const long npix = (long)M * n.g[l].Pp, ms = npix * n.C[l];
        const RnMap m = map_of(n, M, l);
        const int nt = rn_red_nt(m);
        const RnJoin j = join_of(n, M, l, pb, &tb);
        TRYP(FUMI_PH_RN_EW, launch_rn_join_reduce(c.st, j, pb.dout[l], tb.doutd[l], c.sc.rpart, 1));
        TRY(coef_bwd(c, M, l, nt, 5, 0, 1, 2, RCM_TBWD, pb.coef[l][2], V + L[2].offG, HV + L[2].offG, HV + L[2].offB));
        TRY(coef_bwd(c, M, l, nt, 5, 0, 3, 4, RCM_TBWD, pb.coef[l][3], V + L[3].offG, HV + L[3].offG, HV + L[3].offB));
        TRYP(FUMI_PH_RN_EW, launch_rn_join_apply(c.st, j, pb.dout[l], tb.doutd[l], tb.dud[l][2], tb.dud[l][3], 1));
        RnSrc s[4];
        for (int k = 2; k >= 1; --k) {
            TRY(wgrad(c, M, l, L[k], 2, pb.a[l][k - 1], tb.dud[l][k], tb.ad[l][k - 1], pb.du[l][k], HV));
            s[0] = src_of(tb.dud[l][k], ms, frags + L[k].fB, n.FSZ, n.C[l], 9);
            s[1] = src_of(pb.du[l][k], ms, Vfrags + L[k].fB, n.FSZ, n.C[l], 9);
            TRY(conv_plain(c, npix, n.g[l], n.C[l], 2, s, tb.dad[l][k - 1]));
            TRYP(FUMI_PH_RN_EW, launch_rn_bwd_reduce(c.st, m, pb.u[l][k - 1], tb.ud[l][k - 1], pb.da[l][k - 1], tb.dad[l][k - 1],
                                                     pb.coef[l][k - 1], c.sc.rpart, 1));
            TRY(coef_bwd(c, M, l, nt, 3, 0, 1, 2, RCM_TBWD, pb.coef[l][k - 1], V + L[k - 1].offG, HV + L[k - 1].offG, HV + L[k - 1].offB));
            TRYP(FUMI_PH_RN_EW, launch_rn_bwd_apply(c.st, m, pb.u[l][k - 1], tb.ud[l][k - 1], pb.da[l][k - 1], tb.dad[l][k - 1],
                                                    pb.coef[l][k - 1], tb.dud[l][k - 1], 1));
        }
        TRY(wgrad(c, M, l, L[0], xind ? 2 : 1, xin, tb.dud[l][0], xind, pb.du[l][0], HV));
        TRY(wgrad(c, M, l, L[3], xind ? 2 : 1, xin, tb.dud[l][3], xind, pb.du[l][3], HV));
        if (l) {
            s[0] = src_of(tb.dud[l][0], ms, frags + L[0].fB, n.FSZ, n.C[l], 9);
            s[1] = src_of(pb.du[l][0], ms, Vfrags + L[0].fB, n.FSZ, n.C[l], 9);
            s[2] = src_of(tb.dud[l][3], ms, frags + L[3].fB, n.FSZ, n.C[l], 1);
            s[3] = src_of(pb.du[l][3], ms, Vfrags + L[3].fB, n.FSZ, n.C[l], 1);
            TRY(conv_plain(c, npix, n.g[l], n.C[l - 1], 4, s, tb.doutd[l - 1]));
        }
    }
    return rn_join(c);
}

size_t g_rn_budget = 0;                               // workspace budget in bytes for the episode chunking (0: default)

// ---- test hooks (fumi_hip_resnet12_set_option / fumi_hip_rn12_probe) -------------------------------------------------------------------
// probe mode: one lane, and when the meta-batch is a single chunk the buffer table of the step is kept so that tests can read EVERY
// stored intermediate (tests/test_resnet12_probe.py feeds each stage of oracle/resnet12_manual.py the engine's own upstream maps and
// compares that stage's output alone: bf16 decorrelation cannot accumulate).  In this mode the gradient of every inner step and the
// direction of the last Hessian-vector product are kept too (they are overwritten otherwise).  hvp_stop = k: the reverse sweep ends
// after inner step k (its tangent maps, HV and V stay in place for the probe); 0 = the whole sweep.
int g_rn_probe = 0, g_rn_hvp_stop = 0;
constexpr int RN_MAXTAPE = 16;
struct RnProbeTab {
    bool valid; fumi_ws* ws; char* base;
    RnNet n; int T, S, Qn, ntape, nslot, second;
    RnPass tape[RN_MAXTAPE]; RnPass query; RnTan tan;
    float* params; float* heads; float* G; float* dh; float* bar; float* barh; float* HV; float* HVh;
    float* Gsave; float* dhsave; float* Vsave; float* Vhsave; rbf16* img_s; rbf16* img_q;
};
RnProbeTab g_rn_tab;

}  // namespace

struct Rn12Problem : EncProblem { int channels[RN_MAXBLK]; int chunk; };
static_assert(12 * RN_MAXBLK <= ENC_MAXTHETA, "theta table of the problem front");

// bytes of the workspace a chunk of `Bc` episodes needs
static size_t chunk_bytes(RnNet& n, int Bc, const Rn12Problem& p, RnScratch& sc) {
    n.B = Bc;
    const bool grad = p.need_grad != 0, second = grad && p.second_order && p.T > 0;
    const int ntape = second ? p.T : 1, nslot = second ? p.T + 1 : 2;
    const size_t hsz = (size_t)Bc * n.N * (n.F + 1);
    size_t b = scratch_sizes(n, p.S, p.Qn, sc);
    b += ws_align((size_t)Bc * p.S * n.g[0].Pp * 16 * 2) + ws_align((size_t)Bc * p.Qn * n.g[0].Pp * 16 * 2);      // prepared images
    b += (size_t)ntape * pass_bytes(n, p.S, true) + pass_bytes(n, p.Qn, grad);
    if (second) b += tan_bytes(n, p.S);
    b += (size_t)nslot * (ws_align((size_t)Bc * n.PSZ * 4) + ws_align((size_t)Bc * n.FSZ * 2) + ws_align(hsz * 4));
    b += 3 * ws_align((size_t)Bc * n.PSZ * 4) + 3 * ws_align(hsz * 4) + ws_align((size_t)Bc * n.FSZ * 2);        // G, bar, HV | dh, barh, HVh | Vfrags
    b += 2 * ws_align((size_t)n.PSZ * 4);                                                                           // gsum, gacc
    if (g_rn_probe) b += (size_t)(ntape + 1) * (ws_align((size_t)Bc * n.PSZ * 4) + ws_align(hsz * 4));             // Gsave, dhsave | Vsave, Vhsave
    return b + (1u << 16);
}

// ---- machinery shared by the meta-steps and the first-order encoder pair ----------------------------------------------------------------
// Two LANES: the meta-batch's chunks of episodes are independent until their gradients are added, so odd chunks run on a second
// stream (ws->lane, own part of the workspace) beside the even ones on the caller's.  Each lane's kernels alternate between
// MFMA-bound (convolutions, weight gradients: 3/4 of the time) and HBM-bound (element-wise: 1/4) and leave partial last rounds of
// workgroups; two lanes out of phase fill both (measured with two processes of 4 episodes each against one of 8: 15.9 vs 14.1
// episodes/s; in one process at 24 episodes 2 / 3 / 4 lanes: 14.46 / 14.81 / 14.24 -- two by default, FUMI_RN_LANES=n <= 4).
// FUMI_RN_LANES=1 or phase timing: one lane (then the weight gradients fork onto ws->side instead).
constexpr int RN_MAXLANES = 4;
static int rn_lanes(fumi_ws* ws, int B) {
    static const int lanes_env = getenv("FUMI_RN_LANES") ? atoi(getenv("FUMI_RN_LANES")) : 2;
    int lanes = (lanes_env >= 2 && !ws->profiling && !g_rn_probe && B >= 2 && ws->side) ? (lanes_env > RN_MAXLANES ? RN_MAXLANES : lanes_env) : 1;
    return lanes > B ? B : lanes;
}
// workspace budget in bytes (fumi_hip_resnet12_set_budget, else FUMI_RN12_BUDGET_GB, else 200 GB)
static size_t rn_budget() {
    if (g_rn_budget) return g_rn_budget;
    const char* e = getenv("FUMI_RN12_BUDGET_GB");
    return (size_t)((e && atof(e) > 0 ? atof(e) : 200.0) * (double)(1ull << 30));
}
// the largest chunk <= Bc whose bytes (all lanes) fit the budget: total(Bc) is close to linear, start from the estimate, step down
static int rn_fit_chunk(int Bc, size_t budget, const std::function<size_t(int)>& total) {
    const size_t one = total(1);
    const long est = (long)(budget / (one ? one : 1)) + 1;
    if (Bc > est) Bc = (int)(est < 1 ? 1 : est);
    while (Bc > 1 && total(Bc) > budget) --Bc;
    return Bc;
}
// parameter slot of n.B episodes = theta (12 nblk tensors, torch layouts) broadcast to every episode
static int slot_from_theta(hipStream_t st, const RnNet& n, const float* const* theta, float* params) {
    for (int l = 0; l < n.nblk; ++l)
        for (int k = 0; k < RN_NCONV; ++k) {
            const RnLayer& y = n.L[l][k];
            const float* const* th = theta + 12 * l + 3 * k;
            TRY(launch_broadcast(st, n.B, (long)y.Cout * y.Cin_real * y.ntaps, th[0], params + y.offW, n.PSZ));
            TRY(launch_broadcast(st, n.B, y.Cout, th[1], params + y.offG, n.PSZ));
            TRY(launch_broadcast(st, n.B, y.Cout, th[2], params + y.offB, n.PSZ));
        }
    return FUMI_OK;
}
// one summed parameter-slab gradient -> the 12 nblk tensors of g_theta
static int theta_grads_out(hipStream_t st, const RnNet& n, const float* gsum, float* const* g_theta) {
    for (int l = 0; l < n.nblk; ++l)
        for (int k = 0; k < RN_NCONV; ++k) {
            const RnLayer& y = n.L[l][k];
            float* const* g = g_theta + 12 * l + 3 * k;
            HIP_TRY(hipMemcpyAsync(g[0], gsum + y.offW, (size_t)y.Cout * y.Cin_real * y.ntaps * 4, hipMemcpyDeviceToDevice, st));
            HIP_TRY(hipMemcpyAsync(g[1], gsum + y.offG, (size_t)y.Cout * 4, hipMemcpyDeviceToDevice, st));
            HIP_TRY(hipMemcpyAsync(g[2], gsum + y.offB, (size_t)y.Cout * 4, hipMemcpyDeviceToDevice, st));
        }
    return FUMI_OK;
}

int run_rn12_episodes(fumi_ws* ws, hipStream_t st, const Rn12Problem& p) {
    // chunks of episodes on lanes (rn_lanes)
    constexpr int MAXLANES = RN_MAXLANES;
    RnCtx cx[MAXLANES];
    for (int i = 0; i < MAXLANES; ++i) { cx[i].ws = ws; cx[i].st = st; }
    RnCtx& c = cx[0];
    int rc = net_init(c.n, p.B, p.nblk, p.Cin, p.N, p.H, p.W, p.channels);
    if (rc) return rc;
    RnNet& n = c.n;
    if (p.T < 0 || p.S < 1 || p.Qn < 1) return FUMI_EINVAL;
    const bool grad = p.need_grad != 0, second = grad && p.second_order && p.T > 0;
    if (second && p.T > RN_MAXTAPE) return FUMI_ENOTSUP;
    const int ntape = second ? p.T : 1, nslot = second ? p.T + 1 : 2;
    int lanes = rn_lanes(ws, p.B);
    g_rn_tab.valid = false;
    // ---- chunk size: the largest number of episodes whose tapes (one per lane) fit the budget
    const size_t budget = rn_budget();
    int Bc = p.chunk > 0 ? (p.chunk < p.B ? p.chunk : p.B) : (p.B + lanes - 1) / lanes;
    if (p.chunk <= 0) Bc = rn_fit_chunk(Bc, budget, [&](int b) { return (size_t)lanes * chunk_bytes(n, b, p, c.sc); });
    if (Bc >= p.B) lanes = 1;                                             // a single chunk
    const size_t region = ws_align(chunk_bytes(n, Bc, p, c.sc));
    if ((rc = ws_reserve(ws, lanes * region))) return rc;
    // (a high-priority lane stream and GPU_MAX_HW_QUEUES=8 were tried: 1082 / 1068 vs 1063 ms per 16 episodes)
    for (int i = 1; i < lanes; ++i) if (!ws_lane_stream(ws, i)) { lanes = 1; break; }
    // (one lane: its weight gradients fork onto ws->side; with two lanes a stream of weight gradients per lane added nothing --
    // 530.5 vs 524.2 ms per 8-episode step -- and they stay in line)
    if (lanes == 1) { c.side = rn_side_stream(ws); c.ev_fork = ws->ev[0]; c.ev_join = ws->ev[1]; }
    TRY(ws_fork_lanes(ws, st, lanes));
    for (int i = 1; i < lanes; ++i) { cx[i].n = n; cx[i].st = ws->lanes[i - 1]; }
    const size_t F1 = (size_t)n.N * (n.F + 1);
    float* gacc_lane[MAXLANES] = {nullptr, nullptr, nullptr, nullptr};
    fumi_ws* const ws_real = ws;
    // one chunk of episodes [b0, b0 + bc) on its lane's stream, in its lane's half of the workspace
    auto chunk_body = [&](int lane, int b0, int bc, bool first_of_lane, float** gacc_out) -> int {
        RnCtx& c = cx[lane];
        RnNet& n = c.n;
        const hipStream_t st = c.st;                                      // (shadows: everything of this chunk goes to its lane's stream)
        fumi_ws view = *ws_real;                                          // (a private bump pointer per chunk)
        fumi_ws* ws = &view;
        (void)chunk_bytes(n, bc, p, c.sc);                               // (sets n.B = bc and the scratch sizes of this chunk)
        ws->off = (size_t)lane * region;                                 // (ws: this thread's carving view of the workspace)
        float* gsum = ws_f(ws, (size_t)n.PSZ); float* gacc = ws_f(ws, (size_t)n.PSZ);   // first carve: same address in every chunk of a lane
        *gacc_out = gacc;
        c.sc.cpart = ws_f(ws, c.sc.cpart_n); c.sc.rpart = ws_f(ws, c.sc.rpart_n); c.sc.wpart = ws_f(ws, c.sc.wpart_n);
        c.sc.rowl = ws_f(ws, c.sc.rowl_n); c.sc.c2 = ws_f(ws, c.sc.c2_n);
        rbf16* img_s = ws_h(ws, (size_t)bc * p.S * n.g[0].Pp * 16); rbf16* img_q = ws_h(ws, (size_t)bc * p.Qn * n.g[0].Pp * 16);
        std::vector<RnPass> tape(ntape);
        for (int t = 0; t < ntape; ++t) pass_carve(ws, n, p.S, true, tape[t]);
        RnPass query; pass_carve(ws, n, p.Qn, grad, query);
        RnTan tan; memset(&tan, 0, sizeof(tan));
        if (second) tan_carve(ws, n, p.S, tan);
        const size_t hsz = (size_t)bc * F1;
        float* params = ws_f(ws, (size_t)nslot * bc * n.PSZ);
        rbf16* frags = ws_h(ws, (size_t)nslot * bc * n.FSZ);
        float* heads = ws_f(ws, (size_t)nslot * hsz);
        float* G = ws_f(ws, (size_t)bc * n.PSZ); float* bar = ws_f(ws, (size_t)bc * n.PSZ); float* HV = ws_f(ws, (size_t)bc * n.PSZ);
        float* dh = ws_f(ws, hsz); float* barh = ws_f(ws, hsz); float* HVh = ws_f(ws, hsz);
        rbf16* Vfrags = ws_h(ws, (size_t)bc * n.FSZ);
        float* Gsave = nullptr; float* dhsave = nullptr; float* Vsave = nullptr; float* Vhsave = nullptr;
        if (g_rn_probe) {
            Gsave = ws_f(ws, (size_t)ntape * bc * n.PSZ); dhsave = ws_f(ws, (size_t)ntape * hsz);
            Vsave = ws_f(ws, (size_t)bc * n.PSZ); Vhsave = ws_f(ws, hsz);
        }
        if (ws->off > (size_t)(lane + 1) * region || ws->off > ws->cap) return FUMI_ENOMEM;
        if (g_rn_probe && bc == p.B) {                                   // the whole meta-batch in one chunk: keep the buffer table
            RnProbeTab& pt = g_rn_tab;
            pt.ws = ws_real; pt.base = ws_real->base; pt.n = n; pt.T = p.T; pt.S = p.S; pt.Qn = p.Qn; pt.ntape = ntape; pt.nslot = nslot;
            pt.second = second ? 1 : 0;
            for (int t = 0; t < ntape; ++t) pt.tape[t] = tape[t];
            pt.query = query; pt.tan = tan; pt.params = params; pt.heads = heads; pt.G = G; pt.dh = dh; pt.bar = bar; pt.barh = barh;
            pt.HV = HV; pt.HVh = HVh; pt.Gsave = Gsave; pt.dhsave = dhsave; pt.Vsave = Vsave; pt.Vhsave = Vhsave;
            pt.img_s = img_s; pt.img_q = img_q;
            pt.valid = true;
        }
        auto P = [&](int s) { return params + (size_t)s * bc * n.PSZ; };
        auto Fr = [&](int s) { return frags + (size_t)s * bc * n.FSZ; };
        auto Hd = [&](int s) { return heads + (size_t)s * hsz; };
        const float* x_s = p.x_s + (size_t)b0 * p.S * p.Cin * p.H * p.W; const float* x_q = p.x_q + (size_t)b0 * p.Qn * p.Cin * p.H * p.W;
        const int64_t* y_s = p.y_s + (size_t)b0 * p.S; const int64_t* y_q = p.y_q + (size_t)b0 * p.Qn;
        // ---- images -> bf16 padded channels-last (once per chunk), slot 0 = the meta-parameters broadcast to every episode
        TRY(launch_rn_img_prep(st, (long)bc * p.S, p.Cin, n.g[0], x_s, img_s));
        TRY(launch_rn_img_prep(st, (long)bc * p.Qn, p.Cin, n.g[0], x_q, img_q));
        HIP_TRY(hipMemsetAsync(G, 0, (size_t)bc * n.PSZ * 4, st));          // (the slab's padding words stay 0 in every vector derived from G)
        HIP_TRY(hipMemsetAsync(P(0), 0, (size_t)bc * n.PSZ * 4, st));
        HIP_TRY(hipMemsetAsync(HV, 0, (size_t)bc * n.PSZ * 4, st));
        TRY(slot_from_theta(st, n, p.theta, P(0)));
        TRY(frags_of_slot(st, n, P(0), Fr(0)));
        HIP_TRY(hipMemcpyAsync(Hd(0), p.head + (size_t)b0 * F1, hsz * 4, hipMemcpyDeviceToDevice, st));
        // ---- inner loop on the support set
        int cur = 0;
        for (int t = 0; t < p.T; ++t) {
            RnPass& pb = tape[second ? t : 0];
            const int nxt = second ? t + 1 : cur ^ 1;
            TRY(forward_pass(c, p.S, img_s, P(cur), Fr(cur), pb, Hd(cur), y_s, 1.f / p.S, nullptr, nullptr, nullptr, nullptr, nullptr));
            TRY(backward_pass(c, p.S, img_s, Fr(cur), pb, Hd(cur), G, dh));
            if (Gsave) {
                const int ts = second ? t : 0;
                HIP_TRY(hipMemcpyAsync(Gsave + (size_t)ts * bc * n.PSZ, G, (size_t)bc * n.PSZ * 4, hipMemcpyDeviceToDevice, st));
                HIP_TRY(hipMemcpyAsync(dhsave + (size_t)ts * hsz, dh, hsz * 4, hipMemcpyDeviceToDevice, st));
            }
            TRYP(FUMI_PH_RN_EW, launch_axpy(st, (long)bc * n.PSZ, P(cur), -p.alpha, G, P(nxt)));
            TRYP(FUMI_PH_RN_EW, launch_axpy(st, (long)hsz, Hd(cur), -p.alpha, dh, Hd(nxt)));
            TRY(frags_of_slot(st, n, P(nxt), Fr(nxt)));
            cur = nxt;
        }
        // ---- query pass with the adapted parameters
        TRY(forward_pass(c, p.Qn, img_q, P(cur), Fr(cur), query, Hd(cur), y_q, 1.f / p.Qn, p.logits_q + (size_t)b0 * p.Qn * n.N,
                         p.preds_q + (size_t)b0 * p.Qn, p.preds_f ? p.preds_f + (size_t)b0 * p.Qn : nullptr, p.loss_b + b0, p.acc_b + b0));
        if (!grad) return FUMI_OK;
        HIP_TRY(hipMemsetAsync(bar, 0, (size_t)bc * n.PSZ * 4, st));
        TRY(backward_pass(c, p.Qn, img_q, Fr(cur), query, Hd(cur), bar, barh));
        if (second) {
            const int t_stop = g_rn_probe && g_rn_hvp_stop > 0 && g_rn_hvp_stop < p.T ? g_rn_hvp_stop : 0;
            for (int t = p.T - 1; t >= t_stop; --t) {
                if (Vsave) {
                    HIP_TRY(hipMemcpyAsync(Vsave, bar, (size_t)bc * n.PSZ * 4, hipMemcpyDeviceToDevice, st));
                    HIP_TRY(hipMemcpyAsync(Vhsave, barh, hsz * 4, hipMemcpyDeviceToDevice, st));
                }
                TRY(frags_of_slot(st, n, bar, Vfrags));
                TRY(hvp_pass(c, p.S, img_s, Fr(t), tape[t], tan, Hd(t), bar, Vfrags, barh, 1.f / p.S, HV, HVh));
                TRYP(FUMI_PH_RN_EW, launch_axpy(st, (long)bc * n.PSZ, bar, -p.alpha, HV, bar));
                TRYP(FUMI_PH_RN_EW, launch_axpy(st, (long)hsz, barh, -p.alpha, HVh, barh));
            }
        }
        // ---- meta-gradient of the chunk: scaled sum over its episodes, added to the running sum
        TRY(launch_reduce_batched(st, 1, bc, n.PSZ, bar, p.grad_scale, gsum, 0));
        if (first_of_lane) HIP_TRY(hipMemcpyAsync(gacc, gsum, (size_t)n.PSZ * 4, hipMemcpyDeviceToDevice, st));
        else TRY(launch_axpy(st, n.PSZ, gacc, 1.f, gsum, gacc));
        HIP_TRY(hipMemcpyAsync(p.head_bar + (size_t)b0 * F1, barh, hsz * 4, hipMemcpyDeviceToDevice, st));
        return FUMI_OK;
    };
    // chunk k belongs to lane k mod lanes; the chunks are enqueued in order, alternating lanes (a second host thread enqueuing lane 1 on
    // its own changed nothing: 1071 vs 1073 ms per 16 episodes)
    {
        bool first[MAXLANES] = {true, true, true, true};
        int ck = 0;
        for (int b0 = 0; b0 < p.B; b0 += Bc, ++ck) {
            const int bc = p.B - b0 < Bc ? p.B - b0 : Bc, lane = ck % lanes;
            TRY(chunk_body(lane, b0, bc, first[lane], &gacc_lane[lane]));
            first[lane] = false;
        }
    }
    TRY(ws_join_lanes(ws, st, lanes));                                    // the caller's stream waits for the other lanes
    float* gacc = gacc_lane[0];
    for (int i = 1; i < lanes; ++i) if (grad && gacc_lane[i]) TRY(launch_axpy(st, n.PSZ, gacc, 1.f, gacc_lane[i], gacc));
    TRY(launch_episode_stats(st, p.B, p.loss_b, p.acc_b, p.grad_scale, p.stats));
    if (!grad) return FUMI_OK;
    return theta_grads_out(st, n, gacc, p.g_theta);
}

// ------------------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------------------
// the ResNet-12 share of the problem front (after enc_fill_problem): channel counts and the caller's chunk
static void fill_channels(Rn12Problem& p, const int* channels, int chunk) {
    for (int l = 0; l < RN_MAXBLK; ++l) p.channels[l] = l < p.nblk ? channels[l] : 0;
    p.chunk = chunk;
}

// small side allocation that outlives the chunk loop's workspace rewinds: the heads and their adjoints of the WHOLE meta-batch and
// the hypernetwork's activations (owned by the workspace, grown on demand)
namespace {
int side_reserve(fumi_ws* ws, size_t floats, float** out) {
    if (ws->side_cap < floats) {
        HIP_TRY(hipDeviceSynchronize());
        if (ws->side_buf) (void)hipFree(ws->side_buf);
        ws->side_buf = nullptr; ws->side_cap = 0;
        HIP_TRY(hipMalloc((void**)&ws->side_buf, floats * 4 + 1024));
        ws->side_cap = floats;
    }
    *out = ws->side_buf;
    return FUMI_OK;
}
}  // namespace

// ---- first-order encoder pair (AM3's image encoder): encode with the tape kept, backward from the feature adjoints ---------------------
// Every episode's support set and query set is one batch-statistics group.  Workspace layout, the same in both calls (a plan from the
// shapes and the budget, kept in a token by encode so that encode_bwd carves the identical layout):
//   global:       per-episode gradient slabs [2][B][PSZ] (support, query) and their sum [PSZ]
//   lane i:       scratch, theta's parameter / fragment slab for Bc episodes (broadcast at encode; encode_bwd reads no theta), the
//                 backward-only maps (du, da, dout) of a support and a query pass of one chunk; recompute form also: the prepared
//                 images, forward maps and features of one chunk
//   tape (taped form only): chunk k's prepared images and the forward maps (u, a, out, BN tables) of its support and query pass
// TAPED form when the whole meta-batch's tape fits the budget (encode_bwd runs only the backward), else RECOMPUTE (encode keeps no maps;
// encode_bwd runs each chunk's forward again, then its backward).  An episode's arithmetic does not depend on its chunk (the launch
// geometry is priced per RN_BREF episodes), and the gradient is ONE sum over all 2 B per-episode slabs in a fixed order, so both
// forms and every chunking give bit-identical features and gradients.
namespace {
struct RnEncPlan { int lanes, Bc, nchunks, taped; size_t glob, lane, tape, total; };
struct RnEncToken { bool valid; fumi_ws* ws; char* base; int B, S, Qn, Cin, H, W, nblk; int ch[RN_MAXBLK]; RnEncPlan pl; RnDrop drop; };
RnEncToken g_rn_enc = {};
RnEncPlan g_rn_enc_last = {};                         // plan of the last encode (fumi_hip_resnet12_encode_plan)

struct RnEncLane { RnScratch sc; float* params; rbf16* frags; RnPass bs, bq; rbf16* img_s; rbf16* img_q; RnPass fs, fq; float* f; };

size_t enc_tape_bytes(const RnNet& n, int S, int Qn) {
    return ws_align((size_t)n.B * S * n.g[0].Pp * 16 * 2) + ws_align((size_t)n.B * Qn * n.g[0].Pp * 16 * 2) +
           maps_bytes(n, S, true, false) + maps_bytes(n, Qn, true, false);
}
size_t enc_lane_bytes(RnNet n, int Bc, int S, int Qn, bool recompute) {
    n.B = Bc;
    RnScratch sc;
    size_t b = scratch_sizes(n, S, Qn, sc) + ws_align((size_t)Bc * n.PSZ * 4) + ws_align((size_t)Bc * n.FSZ * 2) +
               maps_bytes(n, S, false, true) + maps_bytes(n, Qn, false, true);
    if (recompute) b += enc_tape_bytes(n, S, Qn) + ws_align((size_t)Bc * (S > Qn ? S : Qn) * n.F * 4);
    return b;
}
void enc_plan(fumi_ws* ws, const RnNet& n, int B, int S, int Qn, bool want_tape, RnEncPlan& pl) {
    const size_t budget = rn_budget();
    pl.lanes = rn_lanes(ws, B);
    pl.glob = ws_align((size_t)2 * B * n.PSZ * 4) + ws_align((size_t)n.PSZ * 4);
    const int Bmax = (B + pl.lanes - 1) / pl.lanes;
    RnNet nb = n;
    auto tape_of = [&](int b) { nb.B = b; return ws_align(enc_tape_bytes(nb, S, Qn)); };
    auto taped_total = [&](int b) { return pl.glob + (size_t)pl.lanes * ws_align(enc_lane_bytes(n, b, S, Qn, false)) +
                                           (size_t)((B + b - 1) / b) * tape_of(b); };
    // taped: the largest chunk with which every chunk's tape fits (the backward maps shrink with the chunk, the tape does not)
    int Bc = Bmax;
    while (Bc > 1 && taped_total(Bc) > budget) --Bc;
    pl.taped = want_tape && taped_total(Bc) <= budget;
    if (!pl.taped) {
        const size_t room = budget > pl.glob ? budget - pl.glob : 0;
        Bc = rn_fit_chunk(Bmax, room, [&](int b) { return (size_t)pl.lanes * ws_align(enc_lane_bytes(n, b, S, Qn, true)); });
    }
    if (Bc >= B) pl.lanes = 1;                                            // a single chunk
    pl.Bc = Bc; pl.nchunks = (B + Bc - 1) / Bc;
    pl.lane = ws_align(enc_lane_bytes(n, Bc, S, Qn, !pl.taped));
    pl.tape = pl.taped ? tape_of(Bc) : 0;
    pl.total = pl.glob + (size_t)pl.lanes * pl.lane + (size_t)pl.nchunks * pl.tape + (1u << 16);
}
// lane i's buffers (c.n.B = Bc on return)
int enc_carve_lane(fumi_ws* ws, RnCtx& c, const RnEncPlan& pl, int i, int S, int Qn, RnEncLane& L) {
    fumi_ws view = *ws;
    view.off = pl.glob + (size_t)i * pl.lane;
    RnNet& n = c.n;
    n.B = pl.Bc;
    (void)scratch_sizes(n, S, Qn, c.sc);
    c.sc.cpart = ws_f(&view, c.sc.cpart_n); c.sc.rpart = ws_f(&view, c.sc.rpart_n); c.sc.wpart = ws_f(&view, c.sc.wpart_n);
    c.sc.rowl = ws_f(&view, c.sc.rowl_n); c.sc.c2 = ws_f(&view, c.sc.c2_n);
    L.params = ws_f(&view, (size_t)n.B * n.PSZ); L.frags = ws_h(&view, (size_t)n.B * n.FSZ);
    memset(&L.bs, 0, sizeof(RnPass)); memset(&L.bq, 0, sizeof(RnPass));
    maps_carve(&view, n, S, false, true, L.bs); maps_carve(&view, n, Qn, false, true, L.bq);
    L.img_s = L.img_q = nullptr; L.f = nullptr;
    memset(&L.fs, 0, sizeof(RnPass)); memset(&L.fq, 0, sizeof(RnPass));
    if (!pl.taped) {
        L.img_s = ws_h(&view, (size_t)n.B * S * n.g[0].Pp * 16); L.img_q = ws_h(&view, (size_t)n.B * Qn * n.g[0].Pp * 16);
        maps_carve(&view, n, S, true, false, L.fs); maps_carve(&view, n, Qn, true, false, L.fq);
        L.f = ws_f(&view, (size_t)n.B * (S > Qn ? S : Qn) * n.F);
    }
    return view.off > pl.glob + (size_t)(i + 1) * pl.lane || view.off > ws->cap ? FUMI_ENOMEM : FUMI_OK;
}
// chunk k's forward maps: its tape slot (taped form) or its lane's buffers (recompute form)
int enc_chunk_maps(fumi_ws* ws, const RnNet& n, const RnEncPlan& pl, int k, int S, int Qn, const RnEncLane& L, rbf16** img_s,
                   rbf16** img_q, RnPass& ps, RnPass& pq) {
    if (!pl.taped) { *img_s = L.img_s; *img_q = L.img_q; ps = L.fs; pq = L.fq; return FUMI_OK; }
    fumi_ws view = *ws;
    const size_t o0 = pl.glob + (size_t)pl.lanes * pl.lane + (size_t)k * pl.tape;
    view.off = o0;
    RnNet nb = n; nb.B = pl.Bc;                                           // (every tape slot is laid out for Bc episodes)
    *img_s = ws_h(&view, (size_t)nb.B * S * n.g[0].Pp * 16); *img_q = ws_h(&view, (size_t)nb.B * Qn * n.g[0].Pp * 16);
    memset(&ps, 0, sizeof(RnPass)); memset(&pq, 0, sizeof(RnPass));
    maps_carve(&view, nb, S, true, false, ps); maps_carve(&view, nb, Qn, true, false, pq);
    return view.off > o0 + pl.tape || view.off > ws->cap ? FUMI_ENOMEM : FUMI_OK;
}
void with_bwd_maps(RnPass& p, const RnPass& b) {
    for (int l = 0; l < RN_MAXBLK; ++l) {
        for (int k = 0; k < 4; ++k) p.du[l][k] = b.du[l][k];
        for (int k = 0; k < 2; ++k) p.da[l][k] = b.da[l][k];
        p.dout[l] = b.dout[l];
    }
}
// the drop arguments of a call, checked (FUMI_EINVAL: a rate outside [0, 1), or a block size / map the kernels refuse at a dropped
// block).  With no rate > 0 the result is the all-zero `off` record whatever the block sizes and the seed were.
int enc_drop_args(const RnNet& n, const float* rate, const int* block, unsigned long long seed, RnDrop& d) {
    memset(&d, 0, sizeof(d));
    if (!rate && !block) return FUMI_OK;                                  // the entries without drop
    if (!rate || !block) return FUMI_EINVAL;
    bool on = false;
    for (int l = 0; l < n.nblk; ++l) {
        if (!(rate[l] >= 0.f) || !(rate[l] < 1.f)) return FUMI_EINVAL;
        if (rate[l] > 0.f) {
            int bs; unsigned thr;
            TRY(rn_drop_plan(n.g[l + 1].H, n.g[l + 1].W, rate[l], block[l], &bs, &thr));
            on = true;
        }
    }
    if (!on) return FUMI_OK;
    d.on = true; d.seed = seed;
    for (int l = 0; l < n.nblk; ++l) { d.rate[l] = rate[l]; d.block[l] = block[l]; }
    return FUMI_OK;
}
bool enc_drop_same(const RnDrop& a, const RnDrop& b, int nblk) {
    if (a.on != b.on || a.seed != b.seed) return false;
    for (int l = 0; l < nblk; ++l) if (memcmp(&a.rate[l], &b.rate[l], sizeof(float)) || a.block[l] != b.block[l]) return false;
    return true;
}
bool enc_shape_ok(const RnEncToken& t, fumi_ws* ws, int B, int S, int Qn, int Cin, int H, int W, int nblk, const int* channels) {
    if (!t.valid || t.ws != ws || t.base != ws->base || t.B != B || t.S != S || t.Qn != Qn || t.Cin != Cin || t.H != H || t.W != W ||
        t.nblk != nblk) return false;
    for (int l = 0; l < nblk; ++l) if (t.ch[l] != channels[l]) return false;
    return true;
}
}  // namespace

extern "C" {

// Test hooks.  key 0: probe mode (one lane; a single-chunk step keeps its buffer table for fumi_hip_rn12_probe and the per-step
// gradients / the last Hessian-vector product's direction).  key 1: the reverse sweep stops after inner step `value` (probe mode).
int fumi_hip_resnet12_set_option(int key, int value) {
    if (key == 0) { g_rn_probe = value ? 1 : 0; if (!value) g_rn_tab.valid = false; return FUMI_OK; }
    if (key == 1) { if (value < 0) return FUMI_EINVAL; g_rn_hvp_stop = value; return FUMI_OK; }
    return FUMI_EINVAL;
}

// Copies one stored intermediate of the LAST single-chunk ResNet-12 step run in probe mode out of the workspace.
//   pass 0 .. T-1: the tape of support step `pass` (first order / T = 0: only the last step's tape exists, pass 0);  pass T: the
//   query pass;  pass T + 1: the tangent maps of the last Hessian-vector product (inner step hvp_stop);  pass -1: parameter space.
//   kind (pass >= 0): 0 u[block][idx 0..3: c1, c2, c3, shortcut], 1 a[block][idx 0..1], 2 out[block], 3 du[block][idx], 4 da[block][idx],
//     5 dout[block] (bf16 padded channels-last maps [B][M (H+2)(W+2)][C]); 6 coef[block][idx] fp32 [B][RCF_N][C]; 7 f, 8 df fp32 [B][M][F];
//     9 z, 10 p, 11 dz fp32 [B][M][N] (9 of the query pass: the caller's logits hold it).  The tangent pass has kinds 0-5, 7, 8, 11.
//   kind (pass -1): 0 parameter slot idx [B][PSZ], 1 head slot idx [B][N][F+1], 2 G / 3 dh of inner step idx, 4 bar, 5 bar_h, 6 HV,
//     7 HV_h, 8 V / 9 V_h (direction of the last Hessian-vector product), 10 / 11 prepared support / query images bf16 [B][M Pp][16].
// *n_bytes = its size, *is_bf16 = element type; at most max_bytes are copied.
int fumi_hip_rn12_probe(fumi_ws_t* ws, fumi_stream_t stream, int pass, int kind, int block, int idx, void* out, size_t max_bytes,
                        size_t* n_bytes, int* is_bf16) {
    if (!ws || !out || !n_bytes || !is_bf16 || !g_rn_tab.valid) return FUMI_EINVAL;
    const RnProbeTab& pt = g_rn_tab;
    if (pt.ws != ws || pt.base != ws->base) return FUMI_EINVAL;           // another workspace's step, or the slab has moved since
    const RnNet& n = pt.n;
    const void* src = nullptr; size_t bytes = 0; int bf = 0;
    const size_t hsz = (size_t)n.B * n.N * (n.F + 1), psz = (size_t)n.B * n.PSZ;
    if (pass == -1) {
        switch (kind) {
            case 0: if (idx < 0 || idx >= pt.nslot) return FUMI_EINVAL; src = pt.params + (size_t)idx * psz; bytes = psz * 4; break;
            case 1: if (idx < 0 || idx >= pt.nslot) return FUMI_EINVAL; src = pt.heads + (size_t)idx * hsz; bytes = hsz * 4; break;
            case 2: if (idx < 0 || idx >= pt.ntape) return FUMI_EINVAL; src = pt.Gsave + (size_t)idx * psz; bytes = psz * 4; break;
            case 3: if (idx < 0 || idx >= pt.ntape) return FUMI_EINVAL; src = pt.dhsave + (size_t)idx * hsz; bytes = hsz * 4; break;
            case 4: src = pt.bar; bytes = psz * 4; break;
            case 5: src = pt.barh; bytes = hsz * 4; break;
            case 6: src = pt.HV; bytes = psz * 4; break;
            case 7: src = pt.HVh; bytes = hsz * 4; break;
            case 8: src = pt.Vsave; bytes = psz * 4; break;
            case 9: src = pt.Vhsave; bytes = hsz * 4; break;
            case 10: src = pt.img_s; bytes = (size_t)n.B * pt.S * n.g[0].Pp * 16 * 2; bf = 1; break;
            case 11: src = pt.img_q; bytes = (size_t)n.B * pt.Qn * n.g[0].Pp * 16 * 2; bf = 1; break;
            default: return FUMI_EINVAL;
        }
    } else if (pass == pt.T + 1) {
        if (!pt.second || block < 0 || block >= n.nblk) return FUMI_EINVAL;
        const int M = pt.S;
        const RnTan& tb = pt.tan;
        switch (kind) {
            case 0: if (idx < 0 || idx > 3) return FUMI_EINVAL; src = tb.ud[block][idx]; bytes = map_el(n, M, block) * 2; bf = 1; break;
            case 1: if (idx < 0 || idx > 1) return FUMI_EINVAL; src = tb.ad[block][idx]; bytes = map_el(n, M, block) * 2; bf = 1; break;
            case 2: src = tb.outd[block]; bytes = out_el(n, M, block) * 2; bf = 1; break;
            case 3: if (idx < 0 || idx > 3) return FUMI_EINVAL; src = tb.dud[block][idx]; bytes = map_el(n, M, block) * 2; bf = 1; break;
            case 4: if (idx < 0 || idx > 1) return FUMI_EINVAL; src = tb.dad[block][idx]; bytes = map_el(n, M, block) * 2; bf = 1; break;
            case 5: src = tb.doutd[block]; bytes = out_el(n, M, block) * 2; bf = 1; break;
            case 7: src = tb.fd; bytes = (size_t)n.B * M * n.F * 4; break;
            case 8: src = tb.dfd; bytes = (size_t)n.B * M * n.F * 4; break;
            case 11: src = tb.dzd; bytes = (size_t)n.B * M * n.N * 4; break;
            default: return FUMI_EINVAL;
        }
    } else {
        if (pass < 0 || pass > pt.T || block < 0 || block >= n.nblk) return FUMI_EINVAL;
        if (pass < pt.T && pass >= pt.ntape) return FUMI_EINVAL;
        const RnPass& pb = pass == pt.T ? pt.query : pt.tape[pass];
        const int M = pb.M;
        switch (kind) {
            case 0: if (idx < 0 || idx > 3) return FUMI_EINVAL; src = pb.u[block][idx]; bytes = map_el(n, M, block) * 2; bf = 1; break;
            case 1: if (idx < 0 || idx > 1) return FUMI_EINVAL; src = pb.a[block][idx]; bytes = map_el(n, M, block) * 2; bf = 1; break;
            case 2: src = pb.out[block]; bytes = out_el(n, M, block) * 2; bf = 1; break;
            case 3: if (idx < 0 || idx > 3) return FUMI_EINVAL; src = pb.du[block][idx]; bytes = map_el(n, M, block) * 2; bf = 1; break;
            case 4: if (idx < 0 || idx > 1) return FUMI_EINVAL; src = pb.da[block][idx]; bytes = map_el(n, M, block) * 2; bf = 1; break;
            case 5: src = pb.dout[block]; bytes = out_el(n, M, block) * 2; bf = 1; break;
            case 6: if (idx < 0 || idx > 3) return FUMI_EINVAL; src = pb.coef[block][idx]; bytes = (size_t)n.B * RCF_N * n.C[block] * 4; break;
            case 7: src = pb.f; bytes = (size_t)n.B * M * n.F * 4; break;
            case 8: src = pb.df; bytes = (size_t)n.B * M * n.F * 4; break;
            case 9: src = pb.z; bytes = (size_t)n.B * M * n.N * 4; break;
            case 10: src = pb.p; bytes = (size_t)n.B * M * n.N * 4; break;
            case 11: src = pb.dz; bytes = (size_t)n.B * M * n.N * 4; break;
            default: return FUMI_EINVAL;
        }
    }
    if (!src) return FUMI_ENOTSUP;                                        // (a forward-only pass has no gradient maps)
    *n_bytes = bytes; *is_bf16 = bf;
    const size_t k = bytes < max_bytes ? bytes : max_bytes;
    if (k) HIP_TRY(hipMemcpyAsync(out, src, k, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return FUMI_OK;
}

int fumi_hip_resnet12_set_budget(double gigabytes) { g_rn_budget = gigabytes > 0 ? (size_t)(gigabytes * (double)(1ull << 30)) : 0; return FUMI_OK; }

int fumi_hip_maml_resnet12_step(fumi_ws_t* ws, fumi_stream_t stream,
        int B, int N, int S, int Qn, int Cin, int H, int W, int nblk, const int* channels,
        int T, float alpha, int first_order, int need_grad, float grad_scale, int chunk,
        const float* x_s, const int64_t* y_s, const float* x_q, const int64_t* y_q,
        const float* const* params,
        float* logits_q, int64_t* preds_q, float* preds_q_f32, float* loss_b, float* acc_b, float* stats,
        float* const* g_params) {
    if (!ws || !params || !channels) return FUMI_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(ws->device));
    Rn12Problem p;
    int rc = enc_fill_problem(p, 12, RN_MAXBLK, B, N, S, Qn, Cin, H, W, nblk, T, alpha, need_grad, !first_order, grad_scale, x_s, y_s,
                              x_q, y_q, params, logits_q, preds_q, preds_q_f32, loss_b, acc_b, stats, g_params);
    if (rc) return rc;
    fill_channels(p, channels, chunk);
    const float* Wf = params[12 * nblk]; const float* bf = params[12 * nblk + 1];
    if (!Wf || !bf || (need_grad && (!g_params[12 * nblk] || !g_params[12 * nblk + 1]))) return FUMI_EINVAL;
    const int F = channels[nblk - 1];
    const size_t hsz = (size_t)B * N * (F + 1);
    float* side;
    if ((rc = side_reserve(ws, 2 * head_al(hsz), &side))) return rc;
    float* h = side; float* hbar = side + head_al(hsz);
    if ((rc = launch_broadcast_head(st, B, N, F, Wf, bf, h))) return rc;            // every episode starts from lin_final (maml.py:24-31)
    p.head = h; p.head_bar = hbar;
    if ((rc = run_rn12_episodes(ws, st, p))) { ws_abandon_lanes(ws); return rc; }
    if (!need_grad) return FUMI_OK;
    return launch_split_head_grad(st, B, N, F, hbar, grad_scale, g_params[12 * nblk], g_params[12 * nblk + 1]);
}

int fumi_hip_fumi_resnet12_step(fumi_ws_t* ws, fumi_stream_t stream,
        int B, int N, int S, int Qn, int Cin, int H, int W, int nblk, const int* channels, int Dt, int Ht,
        int T, float alpha, int tanh_head, int need_grad, float grad_scale, int chunk,
        const float* x_s, const int64_t* y_s, const float* x_q, const int64_t* y_q,
        const float* cls_text, const float* text_s,
        const float* const* theta, const float* const* phi,
        float* logits_q, int64_t* preds_q, float* preds_q_f32, float* loss_b, float* acc_b, float* stats,
        float* const* g_theta, float* const* g_phi, float* g_cls_text) {
    if (!ws || !theta || !channels || (!cls_text && !text_s) || Dt < 1 || Ht < 1 || !hyper_head_args_ok(phi, g_phi, need_grad))
        return FUMI_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(ws->device));
    Rn12Problem p;
    int rc = enc_fill_problem(p, 12, RN_MAXBLK, B, N, S, Qn, Cin, H, W, nblk, T, alpha, need_grad, 1, grad_scale, x_s, y_s, x_q, y_q,
                              theta, logits_q, preds_q, preds_q_f32, loss_b, acc_b, stats, g_theta);   // fumi.py:176: second order always
    if (rc) return rc;
    fill_channels(p, channels, chunk);
    const int F = channels[nblk - 1];
    const int R = B * N, H1 = F + 1;
    float* side;
    if ((rc = side_reserve(ws, hyper_head_floats(R, Dt, Ht, H1), &side))) return rc;
    HyperHead hd = hyper_head_carve(side, R, Dt, Ht, H1, tanh_head, phi, cls_text);   // the hypernetwork behind the head (meta_front.h)
    if (!hd.ctext) {                                                     // first support row of each class (fumi.py:207-210)
        if ((rc = launch_class_text_select(st, B, N, S, Dt, text_s, y_s, hd.c, ws->status))) return rc;
        hd.ctext = hd.c;
    }
    if ((rc = hyper_head_fwd_gemm(st, hd))) return rc;
    p.head = hd.h; p.head_bar = hd.hbar;
    if ((rc = run_rn12_episodes(ws, st, p))) { ws_abandon_lanes(ws); return rc; }
    if (!need_grad) return FUMI_OK;
    return hyper_head_bwd_gemm(st, hd, grad_scale, g_phi, g_cls_text);
}

// Forward only: feats [G*M, F] = ResNet12(x [G, M, Cin, H, W]) with the batch statistics of every group of M images taken separately.
int fumi_hip_resnet12_features(fumi_ws_t* ws, fumi_stream_t stream, int G, int M, int Cin, int H, int W, int nblk, const int* channels,
        const float* x, const float* const* theta, float* feats) {
    if (!ws || !x || !theta || !feats || !channels || G < 1 || M < 1) return FUMI_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(ws->device));
    RnCtx c; c.ws = ws; c.st = st;
    int rc = net_init(c.n, G, nblk, Cin, 1, H, W, channels);
    if (rc) return rc;
    const RnNet& n = c.n;
    for (int i = 0; i < 12 * nblk; ++i) if (!theta[i]) return FUMI_EINVAL;
    size_t bytes = scratch_sizes(n, M, M, c.sc) + pass_bytes(n, M, false) + ws_align((size_t)G * M * n.g[0].Pp * 16 * 2) +
                   ws_align((size_t)G * n.PSZ * 4) + ws_align((size_t)G * n.FSZ * 2);
    if ((rc = ws_reserve(ws, bytes))) return rc;
    g_rn_tab.valid = false;
    c.sc.cpart = ws_f(ws, c.sc.cpart_n); c.sc.rpart = ws_f(ws, c.sc.rpart_n); c.sc.wpart = ws_f(ws, c.sc.wpart_n); c.sc.rowl = ws_f(ws, c.sc.rowl_n); c.sc.c2 = ws_f(ws, c.sc.c2_n);
    RnPass pb; pass_carve(ws, n, M, false, pb);
    rbf16* img = ws_h(ws, (size_t)G * M * n.g[0].Pp * 16);
    float* params = ws_f(ws, (size_t)G * n.PSZ); rbf16* frags = ws_h(ws, (size_t)G * n.FSZ);
    TRY(launch_rn_img_prep(st, (long)G * M, Cin, n.g[0], x, img));
    TRY(slot_from_theta(st, n, theta, params));
    TRY(frags_of_slot(st, n, params, frags));
    TRY(forward_pass(c, M, img, params, frags, pb, nullptr, nullptr, 0.f, nullptr, nullptr, nullptr, nullptr, nullptr));
    HIP_TRY(hipMemcpyAsync(feats, pb.f, (size_t)G * M * n.F * 4, hipMemcpyDeviceToDevice, st));
    return FUMI_OK;
}

// ---- first-order encoder pair ---------------------------------------------------------------------------------------------------------
static int rn_encode(fumi_ws_t* ws, fumi_stream_t stream, int B, int S, int Qn, int Cin, int H, int W,
        int nblk, const int* channels, const float* x_s, const float* x_q, const float* const* theta,
        float* feats_s, float* feats_q, int keep_tape, const float* drop_rate, const int* drop_block, unsigned long long drop_seed) {
    if (!ws || !x_s || !x_q || !theta || !feats_s || !feats_q || !channels || B < 1 || S < 1 || Qn < 1) return FUMI_EINVAL;
    if (nblk < 1 || nblk > RN_MAXBLK) return FUMI_EINVAL;
    for (int i = 0; i < 12 * nblk; ++i) if (!theta[i]) return FUMI_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(ws->device));
    g_rn_enc.valid = false; g_rn_tab.valid = false;
    RnCtx c0; c0.ws = ws; c0.st = st;
    int rc = net_init(c0.n, B, nblk, Cin, 1, H, W, channels);
    if (rc) return rc;
    if ((rc = enc_drop_args(c0.n, drop_rate, drop_block, drop_seed, c0.drop))) return rc;
    RnEncPlan pl;
    enc_plan(ws, c0.n, B, S, Qn, keep_tape != 0, pl);
    if ((rc = ws_reserve(ws, pl.total))) return rc;
    for (int i = 1; i < pl.lanes; ++i) if (!ws_lane_stream(ws, i)) return FUMI_EHIP;
    RnCtx cx[RN_MAXLANES]; RnEncLane L[RN_MAXLANES];
    for (int i = 0; i < pl.lanes; ++i) {
        cx[i] = c0;
        cx[i].st = i ? ws->lanes[i - 1] : st;
        if ((rc = enc_carve_lane(ws, cx[i], pl, i, S, Qn, L[i]))) return rc;
    }
    if (pl.lanes == 1) { cx[0].side = rn_side_stream(ws); cx[0].ev_fork = ws->ev[0]; cx[0].ev_join = ws->ev[1]; }
    const size_t img = (size_t)Cin * H * W;
    const int F = c0.n.F;
    auto run = [&]() -> int {
        TRY(ws_fork_lanes(ws, st, pl.lanes));
        for (int i = 0; i < pl.lanes; ++i) {                               // theta's slab of each lane (n.B = Bc)
            TRY(slot_from_theta(cx[i].st, cx[i].n, theta, L[i].params));
            TRY(frags_of_slot(cx[i].st, cx[i].n, L[i].params, L[i].frags));
        }
        for (int k = 0; k < pl.nchunks; ++k) {
            const int lane = k % pl.lanes, b0 = k * pl.Bc, bc = B - b0 < pl.Bc ? B - b0 : pl.Bc;
            RnCtx& c = cx[lane];
            c.n.B = bc;
            rbf16 *img_s, *img_q; RnPass ps, pq;
            TRY(enc_chunk_maps(ws, c.n, pl, k, S, Qn, L[lane], &img_s, &img_q, ps, pq));
            TRY(launch_rn_img_prep(c.st, (long)bc * S, Cin, c.n.g[0], x_s + (size_t)b0 * S * img, img_s));
            TRY(launch_rn_img_prep(c.st, (long)bc * Qn, Cin, c.n.g[0], x_q + (size_t)b0 * Qn * img, img_q));
            ps.f = feats_s + (size_t)b0 * S * F; pq.f = feats_q + (size_t)b0 * Qn * F;     // the pooled features land in the caller's tensors
            c.drop.b0 = b0; c.drop.set = 0;
            TRY(forward_pass(c, S, img_s, L[lane].params, L[lane].frags, ps, nullptr, nullptr, 0.f, nullptr, nullptr, nullptr, nullptr, nullptr));
            c.drop.set = 1;
            TRY(forward_pass(c, Qn, img_q, L[lane].params, L[lane].frags, pq, nullptr, nullptr, 0.f, nullptr, nullptr, nullptr, nullptr, nullptr));
        }
        return ws_join_lanes(ws, st, pl.lanes);
    };
    if ((rc = run())) { ws_abandon_lanes(ws); return rc; }
    g_rn_enc_last = pl;
    if (keep_tape) {
        RnEncToken& t = g_rn_enc;
        t.ws = ws; t.base = ws->base; t.B = B; t.S = S; t.Qn = Qn; t.Cin = Cin; t.H = H; t.W = W; t.nblk = nblk;
        for (int l = 0; l < nblk; ++l) t.ch[l] = channels[l];
        t.pl = pl; t.drop = c0.drop; t.valid = true;
    }
    return FUMI_OK;
}

int fumi_hip_resnet12_encode(fumi_ws_t* ws, fumi_stream_t stream, int B, int S, int Qn, int Cin, int H, int W,
        int nblk, const int* channels, const float* x_s, const float* x_q, const float* const* theta,
        float* feats_s, float* feats_q, int keep_tape) {
    return rn_encode(ws, stream, B, S, Qn, Cin, H, W, nblk, channels, x_s, x_q, theta, feats_s, feats_q, keep_tape, nullptr, nullptr, 0);
}

int fumi_hip_resnet12_encode_drop(fumi_ws_t* ws, fumi_stream_t stream, int B, int S, int Qn, int Cin, int H, int W,
        int nblk, const int* channels, const float* x_s, const float* x_q, const float* const* theta,
        float* feats_s, float* feats_q, int keep_tape, const float* drop_rate, const int* drop_block, uint64_t drop_seed) {
    if (!drop_rate || !drop_block) return FUMI_EINVAL;
    return rn_encode(ws, stream, B, S, Qn, Cin, H, W, nblk, channels, x_s, x_q, theta, feats_s, feats_q, keep_tape, drop_rate, drop_block,
                     drop_seed);
}

static int rn_encode_bwd(fumi_ws_t* ws, fumi_stream_t stream, int B, int S, int Qn, int Cin, int H, int W,
        int nblk, const int* channels, const float* x_s, const float* x_q, const float* dfeats_s,
        const float* dfeats_q, float scale, float* const* g_theta, const float* drop_rate, const int* drop_block,
        unsigned long long drop_seed) {
    if (!ws || !x_s || !x_q || !dfeats_s || !dfeats_q || !g_theta || !channels || nblk < 1 || nblk > RN_MAXBLK) return FUMI_EINVAL;
    const RnEncToken t = g_rn_enc;
    if (!enc_shape_ok(t, ws, B, S, Qn, Cin, H, W, nblk, channels)) return FUMI_EINVAL;     // no tape of this shape in this workspace
    for (int i = 0; i < 12 * nblk; ++i) if (!g_theta[i]) return FUMI_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    RnCtx c0; c0.ws = ws; c0.st = st;
    int rc = net_init(c0.n, B, nblk, Cin, 1, H, W, channels);
    if (rc) return rc;
    if ((rc = enc_drop_args(c0.n, drop_rate, drop_block, drop_seed, c0.drop))) return rc;
    if (!enc_drop_same(c0.drop, t.drop, nblk)) return FUMI_EINVAL;        // the tape was written under another mask (it stays valid)
    HIP_TRY(hipSetDevice(ws->device));
    g_rn_enc.valid = false;                                               // the backward pass overwrites the BN tables of the tape
    const RnEncPlan pl = t.pl;                                            // the layout the forward call left
    if ((rc = ws_reserve(ws, pl.total))) return rc;
    if (ws->base != t.base) return FUMI_EINVAL;
    for (int i = 1; i < pl.lanes; ++i) if (!ws_lane_stream(ws, i)) return FUMI_EHIP;
    RnCtx cx[RN_MAXLANES]; RnEncLane L[RN_MAXLANES];
    for (int i = 0; i < pl.lanes; ++i) {
        cx[i] = c0;
        cx[i].st = i ? ws->lanes[i - 1] : st;
        if ((rc = enc_carve_lane(ws, cx[i], pl, i, S, Qn, L[i]))) return rc;
    }
    if (pl.lanes == 1) { cx[0].side = rn_side_stream(ws); cx[0].ev_fork = ws->ev[0]; cx[0].ev_join = ws->ev[1]; }
    fumi_ws gview = *ws; gview.off = 0;
    const RnNet& n0 = c0.n;
    // per-episode gradient slabs: every entry but the slab padding is written by the backward (the padding is summed, never read)
    float* Gs = ws_f(&gview, (size_t)2 * B * n0.PSZ); float* Gq = Gs + (size_t)B * n0.PSZ;
    float* gsum = ws_f(&gview, (size_t)n0.PSZ);
    const size_t img = (size_t)Cin * H * W;
    const int F = n0.F;
    auto run = [&]() -> int {
        TRY(ws_fork_lanes(ws, st, pl.lanes));
        for (int k = 0; k < pl.nchunks; ++k) {
            const int lane = k % pl.lanes, b0 = k * pl.Bc, bc = B - b0 < pl.Bc ? B - b0 : pl.Bc;
            RnCtx& c = cx[lane];
            c.n.B = bc;
            rbf16 *img_s, *img_q; RnPass ps, pq;
            TRY(enc_chunk_maps(ws, c.n, pl, k, S, Qn, L[lane], &img_s, &img_q, ps, pq));
            with_bwd_maps(ps, L[lane].bs); with_bwd_maps(pq, L[lane].bq);
            ps.df = const_cast<float*>(dfeats_s) + (size_t)b0 * S * F;   // read straight into the average-pool backward
            pq.df = const_cast<float*>(dfeats_q) + (size_t)b0 * Qn * F;
            const float* xs = x_s + (size_t)b0 * S * img; const float* xq = x_q + (size_t)b0 * Qn * img;
            c.drop.b0 = b0; c.drop.set = 0;
            if (!pl.taped) {
                TRY(launch_rn_img_prep(c.st, (long)bc * S, Cin, c.n.g[0], xs, img_s));
                ps.f = L[lane].f;
                TRY(forward_pass(c, S, img_s, L[lane].params, L[lane].frags, ps, nullptr, nullptr, 0.f, nullptr, nullptr, nullptr, nullptr, nullptr));
            }
            TRY(backward_pass(c, S, img_s, L[lane].frags, ps, nullptr, Gs + (size_t)b0 * n0.PSZ, nullptr));
            c.drop.set = 1;
            if (!pl.taped) {
                TRY(launch_rn_img_prep(c.st, (long)bc * Qn, Cin, c.n.g[0], xq, img_q));
                pq.f = L[lane].f;
                TRY(forward_pass(c, Qn, img_q, L[lane].params, L[lane].frags, pq, nullptr, nullptr, 0.f, nullptr, nullptr, nullptr, nullptr, nullptr));
            }
            TRY(backward_pass(c, Qn, img_q, L[lane].frags, pq, nullptr, Gq + (size_t)b0 * n0.PSZ, nullptr));
        }
        TRY(ws_join_lanes(ws, st, pl.lanes));
        // one sum over the 2 B slabs (support and query of every episode) in a fixed order, whatever the chunks and lanes were
        TRY(launch_reduce_batched(st, 1, 2 * B, n0.PSZ, Gs, scale, gsum, 0));
        return theta_grads_out(st, n0, gsum, g_theta);
    };
    if ((rc = run())) { ws_abandon_lanes(ws); return rc; }
    return FUMI_OK;
}

int fumi_hip_resnet12_encode_bwd(fumi_ws_t* ws, fumi_stream_t stream, int B, int S, int Qn, int Cin, int H, int W,
        int nblk, const int* channels, const float* x_s, const float* x_q, const float* dfeats_s,
        const float* dfeats_q, float scale, float* const* g_theta) {
    return rn_encode_bwd(ws, stream, B, S, Qn, Cin, H, W, nblk, channels, x_s, x_q, dfeats_s, dfeats_q, scale, g_theta, nullptr, nullptr, 0);
}

int fumi_hip_resnet12_encode_bwd_drop(fumi_ws_t* ws, fumi_stream_t stream, int B, int S, int Qn, int Cin, int H, int W,
        int nblk, const int* channels, const float* x_s, const float* x_q, const float* dfeats_s,
        const float* dfeats_q, float scale, float* const* g_theta, const float* drop_rate, const int* drop_block, uint64_t drop_seed) {
    if (!drop_rate || !drop_block) return FUMI_EINVAL;
    return rn_encode_bwd(ws, stream, B, S, Qn, Cin, H, W, nblk, channels, x_s, x_q, dfeats_s, dfeats_q, scale, g_theta, drop_rate,
                         drop_block, drop_seed);
}

// DropBlock / dropout of one raw map in place (unit parity of rn12_drop.hip): the count launch, then the apply launch.
// map [B][M (H+2)(W+2)][C] bf16; kept_out [B] int64, scale_out [B] fp32 (device).  rate == 0 still runs both launches (nothing drops).
int fumi_hip_rn12_drop_apply(fumi_ws_t* ws, fumi_stream_t stream, int B, int M, int H, int W, int C, float rate, int block,
        uint64_t seed, int block_index, int set, int b0, void* map_in_out, int64_t* kept_out, float* scale_out) {
    if (!ws || !map_in_out || !kept_out || !scale_out || B < 1 || M < 1 || C < 1) return FUMI_EINVAL;
    int bs; unsigned thr;
    TRY(rn_drop_plan(H, W, rate, block, &bs, &thr));                     // (every refusal before the workspace is touched)
    if (block_index < 0 || set < 0 || set > 1 || b0 < 0) return FUMI_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(ws->device));
    int rc = ws_reserve(ws, ws_align((size_t)B * 4));
    if (rc) return rc;
    unsigned* ticket = (unsigned*)ws_f(ws, (size_t)B);
    return launch_rn_drop(st, B, M, rn_geom(H, W), C, rate, block, seed, block_index, set, b0, (rbf16*)map_in_out,
                          (unsigned long long*)kept_out, ticket, scale_out, true, true);
}

// plan of the last fumi_hip_resnet12_encode: *taped (1 taped, 0 recompute), *chunk (episodes per chunk), *lanes
int fumi_hip_resnet12_encode_plan(int* taped, int* chunk, int* lanes) {
    if (!taped || !chunk || !lanes) return FUMI_EINVAL;
    *taped = g_rn_enc_last.taped; *chunk = g_rn_enc_last.Bc; *lanes = g_rn_enc_last.lanes;
    return FUMI_OK;
}

// ---- unit ops on raw bf16 maps (parity tests of the matrix kernels) ------------------------------------------------------------------
// y [B][M*(H+2)(W+2)][Cout] bf16 = conv_{ntaps}(x [B][M*(H+2)(W+2)][Cin] bf16 padded channels-last, Wt [B][Cout][Cin][k][k] fp32);
// transpose != 0: the input-gradient product (x has Cout channels, y has Cin).  stats (optional) [B][2][Cy]: sum, sum of squares.
int fumi_hip_rn12_conv(fumi_ws_t* ws, fumi_stream_t stream, int B, int M, int H, int W, int Cin, int Cout, int ntaps, int transpose,
        const void* x, const float* Wt, void* y, float* stats) {
    if (!ws || !x || !Wt || !y || B < 1 || M < 1 || H < 1 || W < 1 || (ntaps != 9 && ntaps != 1)) return FUMI_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const long npix = (long)M * rn_geom(H, W).Pp;
    const int Cy = transpose ? Cin : Cout, Cx = transpose ? Cout : Cin;
    const long long xs = npix * Cx, wst = (long long)Cout * Cin * ntaps;
    RnConvPlan plan;                                                   // (every refusal before the clear: a refused call launches nothing)
    TRY(rn_conv_plan(B, Cy, npix, rn_geom(H, W), 1, &Cx, &ntaps, &plan));
    if (transpose && (Cx & 31)) return FUMI_EINVAL;
    HIP_TRY(hipSetDevice(ws->device));
    HIP_TRY(hipMemsetAsync(y, 0, (size_t)B * npix * Cy * 2, st));      // the kernel writes interior pixels only (nothing reads the border of a conv output)
    return fumi_hip_rn12_conv_multi(ws, stream, B, M, H, W, Cy, 1, &Cx, &ntaps, &x, &xs, &Wt, &wst, transpose, nullptr, 0, y, npix * Cy, stats);
}

// The general form (every launch the engine issues: conv_bn / conv_plain): out = sum over 1..4 sources of conv_{ntaps[s]}(x[s], Wt[s]),
// source s with Cin[s] channels and an episode stride x_stride[s] >= npix Cin[s] (elements); Wt[s] fp32 OIHW [Cout][Cin[s]][k][k], or
// with transpose != 0 the forward layer's [Cin[s]][Cout][k][k] whose backward-data copy is multiplied; w_stride[s] = 0: one weight
// set shared by all episodes.  dot (optional, stride dot_stride): the second statistic is sum(out * dot) instead of sum(out^2).
// y (stride y_stride >= npix Cout) is NOT cleared: interior pixels are written, the border is the caller's.  stats (optional)
// [B][2][Cout].  Nothing is launched when an argument is refused.
int fumi_hip_rn12_conv_multi(fumi_ws_t* ws, fumi_stream_t stream, int B, int M, int H, int W, int Cout, int nsrc, const int* Cin,
        const int* ntaps, const void* const* x, const long long* x_stride, const float* const* Wt, const long long* w_stride,
        int transpose, const void* dot, long long dot_stride, void* y, long long y_stride, float* stats) {
    if (!ws || !Cin || !ntaps || !x || !x_stride || !Wt || !w_stride || !y || M < 1 || H < 1 || W < 1) return FUMI_EINVAL;
    const RnGeom g = rn_geom(H, W);
    const long npix = (long)M * g.Pp;
    RnConvPlan plan;
    TRY(rn_conv_plan(B, Cout, npix, g, nsrc, Cin, ntaps, &plan));       // (every refusal of launch_rn_conv, before anything is launched)
    if (y_stride < npix * Cout || (dot && dot_stride < npix * Cout)) return FUMI_EINVAL;
    size_t fel[4] = {0, 0, 0, 0}, need = 0;
    for (int s = 0; s < nsrc; ++s) {
        if (!x[s] || !Wt[s] || x_stride[s] < npix * Cin[s] || w_stride[s] < 0) return FUMI_EINVAL;
        if (transpose && (Cin[s] & 31)) return FUMI_EINVAL;              // (launch_rn_wprep: the layer's forward copy needs Cout % 32 == 0)
        fel[s] = (size_t)ntaps[s] * Cin[s] * Cout;
        if (w_stride[s] && (size_t)w_stride[s] < fel[s]) return FUMI_EINVAL;
        need += (transpose ? 2 : 1) * ws_align((w_stride[s] ? B : 1) * fel[s] * 2);
    }
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(ws->device));
    const int tiles = rn_conv_tiles(npix, g);
    int rc = ws_reserve(ws, need + ws_align((size_t)B * tiles * 2 * Cout * 4));
    if (rc) return rc;
    RnConvArgs a; memset(&a, 0, sizeof(a));
    a.B = B; a.nsrc = nsrc; a.Cout = Cout; a.npix = npix; a.g = g;
    for (int s = 0; s < nsrc; ++s) {
        const int Bw = w_stride[s] ? B : 1;
        rbf16* ff = ws_h(ws, Bw * fel[s]); rbf16* fb = transpose ? ws_h(ws, Bw * fel[s]) : nullptr;
        // the copy that is multiplied is laid out in the LAUNCH's form (one form for all sources)
        if (transpose) TRY(launch_rn_wprep(st, Bw, Cin[s], Cout, Cout, ntaps[s], Wt[s], (long)w_stride[s], ff, fb, (long)fel[s], -1, plan.S16));
        else TRY(launch_rn_wprep(st, Bw, Cout, Cin[s], Cin[s], ntaps[s], Wt[s], (long)w_stride[s], ff, nullptr, (long)fel[s], plan.S16, -1));
        a.src[s] = src_of((const rbf16*)x[s], (long)x_stride[s], transpose ? fb : ff, w_stride[s] ? (long)fel[s] : 0, Cin[s], ntaps[s]);
    }
    for (int s = nsrc; s < 4; ++s) a.src[s] = a.src[0];
    float* part = ws_f(ws, (size_t)B * tiles * 2 * Cout);
    a.out = (rbf16*)y; a.out_stride = (long)y_stride; a.stats = stats ? part : nullptr;
    a.dot = (const rbf16*)dot; a.dot_stride = (long)dot_stride;
    int nt = 0;
    TRY(launch_rn_conv(st, a, &nt));
    if (stats) TRY(launch_reduce_batched(st, B, nt, 2L * Cout, part, 1.f, stats, 2L * Cout));
    return FUMI_OK;
}

// dW [B][Cout][Cin][k][k] fp32 = sum_p dy[p][co] x[p + off][ci]   (x, dy: raw bf16 maps as above)
int fumi_hip_rn12_wgrad(fumi_ws_t* ws, fumi_stream_t stream, int B, int M, int H, int W, int Cin, int Cout, int ntaps,
        const void* x, const void* dy, float* dW) {
    if (M < 1 || H < 1 || W < 1) return FUMI_EINVAL;
    const long npix = (long)M * rn_geom(H, W).Pp;
    return fumi_hip_rn12_wgrad_multi(ws, stream, B, M, H, W, Cin, Cin, Cout, ntaps, 1, 0, x, dy, nullptr, nullptr, npix * Cin, npix * Cout,
                                     dW, (long long)Cout * Cin * ntaps);
}

// The general form (wgrad() of the engine): dW [B][Cout][Cin_real][k][k] (stride dw_stride) = sum over npair (x, dy) pairs; the maps
// have Cin >= Cin_real channels (the image layer: 16 for 3) and episode strides x_stride / dy_stride; nsplit = 0: rn_wgrad_nsplit's
// split of the pixel axis, else that many slabs.
int fumi_hip_rn12_wgrad_multi(fumi_ws_t* ws, fumi_stream_t stream, int B, int M, int H, int W, int Cin, int Cin_real, int Cout, int ntaps,
        int npair, int nsplit, const void* x0, const void* dy0, const void* x1, const void* dy1, long long x_stride, long long dy_stride,
        float* dW, long long dw_stride) {
    if (!ws || !x0 || !dy0 || !dW || M < 1 || H < 1 || W < 1 || Cin < 16 || Cout < 32 || Cin_real < 1 || Cin_real > Cin) return FUMI_EINVAL;
    if (nsplit < 0 || nsplit > 512 || (npair == 2 && (!x1 || !dy1))) return FUMI_EINVAL;
    const RnGeom g = rn_geom(H, W);
    RnWgradArgs a; memset(&a, 0, sizeof(a));
    a.B = B; a.npair = npair; a.Cin = Cin; a.Cout = Cout; a.ntaps = ntaps; a.npix = (long)M * g.Pp; a.g = g;
    RnWgradPlan plan;
    a.nsplit = nsplit ? nsplit : (B >= 1 ? rn_wgrad_nsplit(B, a.npix, Cin, Cout) : 1);
    TRY(rn_wgrad_plan(B, npair, Cin, Cout, ntaps, a.nsplit, a.npix, g, &plan));       // (every refusal of launch_rn_wgrad, before anything is launched)
    if (x_stride < a.npix * Cin || dy_stride < a.npix * Cout || dw_stride < (long long)Cout * Cin_real * ntaps) return FUMI_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(ws->device));
    const int Ci32 = (Cin + 31) / 32 * 32;
    int rc = ws_reserve(ws, ws_align((size_t)B * a.nsplit * ntaps * Cout * Ci32 * 4));
    if (rc) return rc;
    a.part = ws_f(ws, (size_t)B * a.nsplit * ntaps * Cout * Ci32);
    a.x[0] = (const rbf16*)x0; a.dy[0] = (const rbf16*)dy0; a.x[1] = (const rbf16*)x1; a.dy[1] = (const rbf16*)dy1;
    a.x_stride = (long)x_stride; a.dy_stride = (long)dy_stride;
    TRY(launch_rn_wgrad(st, a));
    return launch_rn_wgrad_reduce(st, B, a.nsplit, ntaps, Cout, Cin, Cin_real, a.part, dW, (long)dw_stride);
}

// ---- unit ops of the element-wise passes on raw buffers (tests/rn12_ew_forms.py) ---------------------------------
// Every launcher of rn12_ew.hip as the engine calls it: maps bf16 [B][M (H+2)(W+2)][C] padded channels-last, coefficient tables fp32
// [B][RCF_N][C], partial sums fp32 [B][nt][K][C] (nt: fumi_hip_rn12_ew_query).  Every refusal comes before anything is launched.
static int ew_map_of(int B, int M, int H, int W, int C, int kind, int tangent, int form, RnMap* m) {
    RnEwPlan p;
    TRY(rn_ew_plan(B, M, H, W, C, kind, tangent, form, &p));
    m->B = B; m->M = M; m->C = C; m->g = rn_geom(H, W);
    return FUMI_OK;
}

// out = lrelu(A u + C0); ud != NULL: the tangent form
int fumi_hip_rn12_ew_act(fumi_ws_t* ws, fumi_stream_t stream, int B, int M, int H, int W, int C, const void* u, const void* ud,
        const float* coef, void* out) {
    if (!ws || !u || !coef || !out) return FUMI_EINVAL;
    RnMap m;
    TRY(ew_map_of(B, M, H, W, C, RN_EW_ACT, ud != nullptr, 0, &m));
    HIP_TRY(hipSetDevice(ws->device));
    return launch_rn_act((hipStream_t)stream, m, (const rbf16*)u, (const rbf16*)ud, coef, (rbf16*)out);
}

// apply = 0: the partial sums of the BN backward -> out fp32 [B][nt][K = 2 | 3][C]; apply = 1: du -> out bf16 map
int fumi_hip_rn12_ew_bwd(fumi_ws_t* ws, fumi_stream_t stream, int B, int M, int H, int W, int C, int apply, int tangent, const void* u,
        const void* ud, const void* da, const void* dad, const float* coef, void* out) {
    if (!ws || !u || !da || !coef || !out || apply < 0 || apply > 1 || tangent < 0 || tangent > 1) return FUMI_EINVAL;
    if (tangent && (!ud || !dad)) return FUMI_EINVAL;
    RnMap m;
    TRY(ew_map_of(B, M, H, W, C, apply ? RN_EW_BWD_APPLY : RN_EW_BWD_REDUCE, tangent, 0, &m));
    HIP_TRY(hipSetDevice(ws->device));
    hipStream_t st = (hipStream_t)stream;
    if (apply) return launch_rn_bwd_apply(st, m, (const rbf16*)u, (const rbf16*)ud, (const rbf16*)da, (const rbf16*)dad, coef, (rbf16*)out, tangent);
    return launch_rn_bwd_reduce(st, m, (const rbf16*)u, (const rbf16*)ud, (const rbf16*)da, (const rbf16*)dad, coef, (float*)out, tangent);
}

// pass_ 0: o = maxpool(lrelu(BN3(u3) + BNs(us))) -> out0 bf16 [B][M (H/2+2)(W/2+2)][C]; 1: partial sums -> out0 fp32 [B][nt][K = 3 | 5][C];
// 2: du3 -> out0, dus -> out1 (bf16 maps); form 1 (pass 2, plain): the cell form
int fumi_hip_rn12_ew_join(fumi_ws_t* ws, fumi_stream_t stream, int B, int M, int H, int W, int C, int pass_, int tangent, int form,
        const void* u3, const void* us, const void* u3d, const void* usd, const float* coef3, const float* coefs, const void* dout,
        const void* doutd, void* out0, void* out1) {
    if (!ws || !u3 || !us || !coef3 || !coefs || !out0 || pass_ < 0 || pass_ > 2 || tangent < 0 || tangent > 1) return FUMI_EINVAL;
    if (tangent && (!u3d || !usd)) return FUMI_EINVAL;
    if (pass_ && (!dout || (tangent && !doutd))) return FUMI_EINVAL;
    if (pass_ == 2 && !out1) return FUMI_EINVAL;
    RnJoin j; memset(&j, 0, sizeof(j));
    TRY(ew_map_of(B, M, H, W, C, pass_ == 0 ? RN_EW_JOIN_FWD : pass_ == 1 ? RN_EW_JOIN_REDUCE : RN_EW_JOIN_APPLY, tangent, form, &j.m));
    j.Ho = H / 2; j.Wo = W / 2; j.gn = rn_geom(j.Ho, j.Wo);
    j.u3 = (const rbf16*)u3; j.us = (const rbf16*)us; j.coef3 = coef3; j.coefs = coefs; j.u3d = (const rbf16*)u3d; j.usd = (const rbf16*)usd;
    HIP_TRY(hipSetDevice(ws->device));
    hipStream_t st = (hipStream_t)stream;
    if (pass_ == 0) return launch_rn_join_fwd(st, j, (rbf16*)out0, tangent);
    if (pass_ == 1) return launch_rn_join_reduce(st, j, (const rbf16*)dout, (const rbf16*)doutd, (float*)out0, tangent);
    return launch_rn_join_apply(st, j, (const rbf16*)dout, (const rbf16*)doutd, (rbf16*)out0, (rbf16*)out1, tangent, form);
}

// the coefficient pass (RnCoefArgs, rn12.h) with caller-given slab count, slices and strides; scratch (optional): at least
// rn_coef_scratch_floats = B ceil(nt / 64) K C floats (fumi_hip_rn12_coef_query), NULL: rn_coef_kernel alone whatever nt
int fumi_hip_rn12_ew_coef(fumi_ws_t* ws, fumi_stream_t stream, int B, int C, int mode, int nt, int K, int k0, int k1, int k2, float n,
        const float* part, float* coef, const float* g, const float* beta, long long pstride, const float* gd, const float* betad,
        long long dstride, float* dg, float* dbeta, long long gstride, float* scratch) {
    if (!ws || !part || !coef || mode < RCM_FWD || mode > RCM_TBWD || K < 1 || !(n > 0.f)) return FUMI_EINVAL;
    if (k0 < 0 || k0 >= K || k1 < 0 || k1 >= K || k2 < 0 || k2 >= K) return FUMI_EINVAL;
    if (mode == RCM_FWD && (!g || !beta || pstride < C)) return FUMI_EINVAL;
    if (mode == RCM_TFWD && (!gd || !betad || dstride < C)) return FUMI_EINVAL;
    if ((mode == RCM_BWD || mode == RCM_TBWD) && (!dg || !dbeta || gstride < C)) return FUMI_EINVAL;
    if (mode == RCM_TBWD && (!gd || dstride < C)) return FUMI_EINVAL;
    RnCoefPlan p;
    TRY(rn_coef_plan(B, nt, K, C, scratch != nullptr, &p));
    RnCoefArgs a; memset(&a, 0, sizeof(a));
    a.B = B; a.C = C; a.mode = mode; a.nt = nt; a.K = K; a.k0 = k0; a.k1 = k1; a.k2 = k2; a.n = n; a.part = part; a.coef = coef;
    a.g = g; a.beta = beta; a.pstride = (long)pstride; a.gd = gd; a.betad = betad; a.dstride = (long)dstride;
    a.dg = dg; a.dbeta = dbeta; a.gstride = (long)gstride;
    HIP_TRY(hipSetDevice(ws->device));
    return launch_rn_coef((hipStream_t)stream, a, scratch);
}

// adjoint = 0: f fp32 [BM][C] = mean over the interior of in bf16 [BM][(H+2)(W+2)][C]; 1: out bf16 map = in fp32 [BM][C] / (H W), border 0
int fumi_hip_rn12_ew_avgpool(fumi_ws_t* ws, fumi_stream_t stream, int BM, int H, int W, int C, int adjoint, const void* in, void* out) {
    if (!ws || !in || !out || adjoint < 0 || adjoint > 1) return FUMI_EINVAL;
    RnEwPlan p;
    TRY(rn_ew_plan(1, BM, H, W, C, adjoint ? RN_EW_AVGPOOL_BWD : RN_EW_AVGPOOL, 0, 0, &p));
    HIP_TRY(hipSetDevice(ws->device));
    if (adjoint) return launch_rn_avgpool_bwd((hipStream_t)stream, BM, C, rn_geom(H, W), (const float*)in, (rbf16*)out);
    return launch_rn_avgpool((hipStream_t)stream, BM, C, rn_geom(H, W), (const rbf16*)in, (float*)out);
}

// img fp32 [BM][Cin][H][W] -> out bf16 [BM][(H+2)(W+2)][16], channels Cin..15 and the border zero; Cin outside 1..8: FUMI_EINVAL
int fumi_hip_rn12_ew_img_prep(fumi_ws_t* ws, fumi_stream_t stream, int BM, int Cin, int H, int W, const float* img, void* out) {
    if (!ws || !img || !out) return FUMI_EINVAL;
    RnEwPlan p;
    TRY(rn_ew_plan(1, BM, H, W, Cin, RN_EW_IMG_PREP, 0, 0, &p));
    HIP_TRY(hipSetDevice(ws->device));
    return launch_rn_img_prep((hipStream_t)stream, BM, Cin, rn_geom(H, W), img, (rbf16*)out);
}

}  // extern "C"
