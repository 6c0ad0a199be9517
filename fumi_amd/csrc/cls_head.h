// What the classification heads of --model pretrain share (clshead.hip: hard, soft-target and distillation head; coshead.hip: cosine
// classifier): the tile constants, the dims and soft-target structs, the host's checks, launch dimensions and
// soft-target builder, and the one kernel block that moved without changing a kernel's code, the tile sums.  A block is here only if
// every kernel it touches compiles to the instruction stream it had with the block as a copy (profiles/cls_head_shared/).
// NOT here, copies in their kernels, each marked "(cls_head.h: a copy)": the row arg-max, the row sums, the label rule and the soft
// target of the rows kernels, and the final sum over the tiles and the column sum of the weight-gradient kernels.  Through a helper
// each of them changed the instruction stream of a kernel (block placement and register allocation in the rows kernels, the sense
// of a back edge or two address instructions in the weight-gradient kernels), and those kernels are the heads' time.
//
// What every head promises, in that block and in the copies:
//   - every sum has a fixed order (MFMA chains over k, butterflies inside a 16-lane group, index-ordered loops across rows and tiles,
//     strided sums added in index order): equal inputs give equal bits;
//   - the prediction is the FIRST arg-max, as torch.max returns it; a row of NaNs predicts class 0;
//   - a label outside [0, C) sets FUMI_ST_LABEL_RANGE: its row adds nothing to the loss, the counts or any gradient while the divisor
//     stays M;
//   - no floating-point atomics: the only atomic is the OR into the status word.
#pragma once
#include "common.h"
#include <initializer_list>

constexpr int CL_TM = 16;          // rows per workgroup of the rows kernel, classes per workgroup of the weight-gradient kernel
constexpr int CL_NB = 128;         // output columns of one wg_mm call: 8 MFMA tiles = one pass of 4 waves x 2 tiles
constexpr int CL_MM = 16384;       // floats of LDS the products stage their operands in
constexpr int CL_MAXTILE = 4096 / CL_TM;   // stride of the tile sums: part[k * CL_MAXTILE + tile]

// ---- host side ---------------------------------------------------------------------------------------------------------------------
struct ClsHead {
    int M, F, C, ldz, ntile, train;
    float gs;                      // grad_scale / M
};
struct ClsSoft {                   // the soft target of a row: t[c] = base + wa [c == y_a] + wb [c == y_b]
    const int64_t* yb;
    float wa, wb, base;            // (1 - eps) lam, (1 - eps) (1 - lam), eps / C
};
static inline void cl_dims_fill(ClsHead& d, int M, int F, int C, int train, float grad_scale) {
    d.M = M; d.F = F; d.C = C; d.ldz = ((C + 15) & ~15) + 4; d.ntile = (M + CL_TM - 1) / CL_TM; d.train = train;
    d.gs = grad_scale / (float)M;
}
// the three gradient pointers come together or not at all: 1 training form, 0 forward form, -1 neither
static inline int cl_grad_form(const void* dfeats, const void* gW, const void* gparam) {
    const int ngrad = (dfeats ? 1 : 0) + (gW ? 1 : 0) + (gparam ? 1 : 0);
    return ngrad == 3 ? 1 : ngrad == 0 ? 0 : -1;
}
// The refusals of every entry in their fixed order, after the entry's own (soft target, teacher): FUMI_EINVAL without a workspace,
// for a null among `need` or a dimension below 1, FUMI_EINVAL for one or two gradients (`form` < 0), FUMI_ENOTSUP outside the limits.
static inline int cl_args_check(const fumi_ws_t* ws, int M, int F, int C, int form, std::initializer_list<const void*> need) {
    if (!ws || M < 1 || F < 1 || C < 1) return FUMI_EINVAL;
    for (const void* p : need) if (!p) return FUMI_EINVAL;
    if (form < 0) return FUMI_EINVAL;
    if (M > 4096 || F % 32 != 0 || F < 32 || F > 2048 || C < 2 || C > 1024) return FUMI_ENOTSUP;
    return FUMI_OK;
}
// workgroups of the weight-gradient launch: one per [16 classes x 128 features] block in the training form, and the one that adds the
// tile sums
static inline int cl_feature_blocks(int F) { return (F + CL_NB - 1) / CL_NB; }
static inline int cl_wgrad_grid(const ClsHead& d) { return (d.train ? ((d.C + CL_TM - 1) / CL_TM) * cl_feature_blocks(d.F) : 0) + 1; }
// the soft target of label smoothing `smoothing` and the two-label mix `lam` (y_b null: y_b = y_a, and lam must be 1); FUMI_EINVAL
// outside smoothing in [0, 1), lam in [0, 1]
static inline int cl_soft_fill(ClsSoft& s, const int64_t* y_a, const int64_t* y_b, float lam, float smoothing, int C) {
    if (!(smoothing >= 0.f && smoothing < 1.f) || !(lam >= 0.f && lam <= 1.f) || (!y_b && lam != 1.f)) return FUMI_EINVAL;
    const float u = 1.f - lam, keep = 1.f - smoothing;
    s.yb = y_b ? y_b : y_a; s.wa = keep * lam; s.wb = keep * u; s.base = smoothing / (float)C;
    return FUMI_OK;
}

// ---- tile sums ---------------------------------------------------------------------------------------------------------------------
// rl [K][16] (row scalars of this workgroup's tile, after a barrier) -> part[k * CL_MAXTILE + tile], rows in index order, by thread 0
template <int K>
__device__ __forceinline__ void cl_tile_part(const float* rl, float* part, int k0 = 0) {
    if (threadIdx.x == 0) {
        float a[K];
#pragma unroll
        for (int k = 0; k < K; ++k) a[k] = 0.f;
        for (int r = 0; r < CL_TM; ++r) {
#pragma unroll
            for (int k = 0; k < K; ++k) a[k] += rl[16 * (k0 + k) + r];
        }
#pragma unroll
        for (int k = 0; k < K; ++k) part[(k0 + k) * CL_MAXTILE + blockIdx.x] = a[k];
    }
}
