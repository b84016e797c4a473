// kpconv.h -- the internal interface of the KPConv gather, declared here and nowhere else: the descriptor of one gather
// (KpconvCall), the one entry that runs it (kpconv_run, kpconv.hip), and the three host rules that kpconv.hip and
// kpconv_ex.hip share -- where the support records live in a workspace (KpWs), how a launch is cut into channel blocks and
// workgroups (kpconv_plan) and when the float4 kernels apply (kpconv_vec_ok).  The forward runner and the transposed
// backward fill a KpconvCall; the extern "C" entries of kpconv.hip do the same with their arguments.
#pragma once
#include "common.h"

namespace pcrcg {

enum class KpForm {
    f32,          // wf [nq, 15 * cin] fp32 (cin = 1: rows of c1_ld floats)
    bf16,         // bf16 feature storage: the gathers read x_bf16, the pack's rounded copy of x, and write wf_bf16
    c1_fused      // cin = 1, the whole layer in one kernel: y = (wf @ wt^T) / n_q and its column sums, no wf in memory
};

// One rigid / linear / sum gather: wf[q, k, :] = sum_h w[q, h, k] x[idx[q, h], :] and inv_n[q] = 1 / n_q.
struct KpconvCall {
    const float* q_pts = nullptr;       // [nq, 3]
    int nq = 0;
    const float* s_pts = nullptr;       // [ns, 3]
    int ns = 0;                         // also the shadow index of the table
    const int64_t* idx = nullptr;       // [nq, h] in rows of ld_idx
    int h = 0, ld_idx = 0;
    const float* x = nullptr;           // [ns, cin] fp32 in every form (the pack reads it)
    int cin = 0;
    const float* kp = nullptr;          // [15, 3]
    float extent = 0.f;
    float* wf = nullptr;                // KpForm::f32 only
    float* inv_n = nullptr;             // [nq]
    void* ws = nullptr;                 // pcrcg_kpconv_ws_bytes(ns)
    size_t ws_bytes = 0;
    hipStream_t st = nullptr;
    KpForm form = KpForm::f32;
    bool pack = true;                   // build the support records in ws first; false: they are there (instnorm_apply_pack)
    const int* walk = nullptr;          // the queries' processing order (walk.hip), NULL: index order
    int c1_ld = 0;                      // cin = 1: floats per wf row, 15 (0 means 15) or 16 (15 + a zero)
    unsigned short* x_bf16 = nullptr;   // KpForm::bf16: [ns, cin] scratch and [nq, 15 * cin] output, 8-byte aligned
    unsigned short* wf_bf16 = nullptr;
    const float* wt = nullptr;          // KpForm::c1_fused: weights [cout, 16] (K-contiguous, the 16th column unused),
    int cout = 0;                       //   y [nq, cout] in rows of ld_y, and sums [2][cout] f64 (zeroed by the caller),
    float* y = nullptr;                 //   to which the column sums and sums of squares of y are ADDED
    int ld_y = 0;
    double* sums = nullptr;
};

// kpconv.hip.  Checks the call, carves the workspace, packs if asked, plans and launches.  nq == 0 is PCRCG_OK before any
// pointer but wt is looked at (KpForm::bf16 wants ns >= 1 even then); a workspace that is too small is PCRCG_EWORKSPACE
// before any launch.
int kpconv_run(const KpconvCall& c);
// the widths and weights KpForm::c1_fused serves (everything else keeps gather + product)
bool kpconv_c1_fused_ok(int cout, const float* wt);

// The layout pcrcg_kpconv_ws_bytes(ns) sizes: row-positive flags, then the packed (x, y, z, flag) support records.
struct KpWs { unsigned char* pos; float4* pk; };
int kpconv_ws(void* ws, size_t ws_bytes, int ns, KpWs* out);      // PCRCG_EWORKSPACE: too small
inline float4* kpconv_pk_ptr(void* ws, size_t ws_bytes, int ns) {
    KpWs w;
    return kpconv_ws(ws, ws_bytes, ns, &w) == PCRCG_OK ? w.pk : nullptr;
}
// kpconv.hip: flags and records of x into w (x_bf16 != NULL: also the bf16 round-to-nearest-even copy of x, [ns, cin])
int kpconv_pack(const float* x, int ns, int cin, const float* s_pts, const KpWs& w, hipStream_t st,
                unsigned short* x_bf16 = nullptr);

// How a launch of one wavefront per (query, channel chunk) is cut: nb 64-channel blocks per wavefront, nchunk chunks per
// query, workgroups of four wavefronts.
struct KpPlan { int nb, nchunk, blocks; bool tail; };
// workgroups for `waves` wavefronts of work: at most 8192; with a walk, eight XCD ranges of at most ceil(nq / 8) queries
// each and the same number of workgroups for every range (`waves` is then the work of one range)
inline constexpr int kpconv_blocks(long waves, bool walk = false) {
    const long b = (waves + 3) / 4, cap = walk ? 8192 / 8 : 8192;
    return (int)(walk ? 8 * (b > cap ? cap : b) : (b > cap ? cap : b));
}
// As many channel blocks per wavefront (4, 2, 1) as divide the row and keep about 16k wavefronts in the grid.  tail (fp32
// storage only: allow_tail): cin = 64 nb + 4 -- PCR-CG's 129 channels in rows of 132 -- takes ONE wavefront per query, the
// last float4 on the vector units.
inline constexpr KpPlan kpconv_plan(int nq, int cin, bool walk, bool allow_tail) {
    const bool tail = allow_tail && (cin == 68 || cin == 132);
    const int nblk = tail ? cin / 64 : (cin + 63) / 64;
    int nb = nblk >= 4 ? 4 : (nblk >= 2 ? 2 : 1);
    while (!tail && nb > 1 && ((long)nq * ((nblk + nb - 1) / nb) < 16384 || nblk % nb != 0)) nb >>= 1;
    const int nchunk = (nblk + nb - 1) / nb;
    return {nb, nchunk, kpconv_blocks((long)(walk ? (nq + 7) / 8 : nq) * nchunk, walk), tail};
}
constexpr bool kp_plan_is(KpPlan p, int nb, int nchunk, int blocks, bool tail) {
    return p.nb == nb && p.nchunk == nchunk && p.blocks == blocks && p.tail == tail;
}
static_assert(kp_plan_is(kpconv_plan(1000, 64, false, true), 1, 1, 250, false));
static_assert(kp_plan_is(kpconv_plan(1000, 64, true, true), 1, 1, 256, false));
static_assert(kp_plan_is(kpconv_plan(16500, 128, false, true), 2, 1, 4125, false));
static_assert(kp_plan_is(kpconv_plan(16500, 128, true, true), 2, 1, 4128, false));
static_assert(kp_plan_is(kpconv_plan(8200, 256, false, true), 2, 2, 4100, false));
static_assert(kp_plan_is(kpconv_plan(16500, 256, false, true), 4, 1, 4125, false));
static_assert(kp_plan_is(kpconv_plan(8200, 512, false, true), 4, 2, 4100, false));
static_assert(kp_plan_is(kpconv_plan(60000, 192, false, true), 1, 3, 8192, false));
static_assert(kp_plan_is(kpconv_plan(60000, 192, true, true), 1, 3, 8192, false));
static_assert(kp_plan_is(kpconv_plan(20000, 132, false, true), 2, 1, 5000, true));
static_assert(kp_plan_is(kpconv_plan(20000, 68, false, true), 1, 1, 5000, true));
static_assert(kp_plan_is(kpconv_plan(20000, 132, false, false), 1, 3, 8192, false));

// the float4 kernels apply: whole float4s per row and 16-byte aligned rows (else the scalar kernels)
inline bool kpconv_vec_ok(int cin, const void* x, const void* out) {
    return (cin % 4 == 0) && ((reinterpret_cast<uintptr_t>(x) & 15) == 0) && ((reinterpret_cast<uintptr_t>(out) & 15) == 0);
}

}  // namespace pcrcg
