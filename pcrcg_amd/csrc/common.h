// common.h -- shared host-side helpers of libpcrcg_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <map>
#include <mutex>

#include "pcrcg.h"

namespace pcrcg {

void set_error(const char* fmt, ...);

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// Bump allocator over the caller's workspace; every carve is 256-byte aligned.
struct Carver {
    char* base;
    size_t cap;
    size_t off = 0;
    Carver(void* ws, size_t bytes) : base(static_cast<char*>(ws)), cap(bytes) {}
    template <typename T>
    T* take(size_t count) {
        size_t bytes = (count * sizeof(T) + 255) & ~size_t(255);
        T* p = reinterpret_cast<T*>(base + off);
        off += bytes;
        return p;
    }
    bool ok() const { return off <= cap; }
};
inline size_t carve_bytes(size_t count, size_t elem) { return (count * elem + 255) & ~size_t(255); }

// Exclusive prefix sum of int32 (device-wide, any n >= 0).  out may alias in.  If total != nullptr
// the grand total is stored there.  ws: scan_ws_bytes(n).
size_t scan_ws_bytes(int n);
int exclusive_scan_i32(const int* in, int* out, int n, int* total, void* ws, hipStream_t stream);

constexpr int kWave = 64;

// max(a, b) as torch.max, F.relu and F.max_pool2d compute it: NaN when either operand is NaN (fmaxf returns the other one).
// The rule of include/pcrcg.h "Non-finite values"; one v_maximum3_f32 on gfx950.
__device__ __forceinline__ float max_nan(float a, float b) { return __builtin_elementwise_maximum(a, b); }

// pointops.hip: InstanceNorm + LeakyReLU that also leaves the KPConv support records of its output (kpconv.hip: pk)
bool instnorm_pack_ok(int c, int ldx, int ldy);
int instnorm_apply_pack(const float* x, int n, int c, int ldx, const float* stats, const double* sums, double count, float eps,
                        float slope, float* y, int ldy, const float* s_pts, float4* pk, hipStream_t st);
// pointops.hip, for gnn.hip: finish a [chunks][2][c] fp64 partial buffer (colstats_ws_bytes(c), at most colstats_chunks()
// chunks) into (mean, rstd) pairs
size_t colstats_ws_bytes(int c);
int colstats_finalize(const double* partial, int nchunks, int c, double count, float eps, float* stats,
                      hipStream_t st);
int colstats_chunks();

// The deterministic debug mode's scratch: one device buffer per stream, kept until pcrcg_debug_release() (scan.hip) frees
// those of every instance.  An instance is a namespace-scope object of the file that uses it (gemm_x6.hip: the split-K
// partial tiles, conv2d.hip: the BatchNorm partial sums, trainops.hip: the fixed-point accumulators).
class StreamScratch {
public:
    // cleared: a newly allocated buffer is handed out zeroed, by a memset enqueued on the stream it was asked for
    explicit StreamScratch(bool cleared = false);
    // >= bytes of device memory for work enqueued on st.  Too small: the stream is drained, the old buffer freed and
    // bytes + slack allocated (a debugging mode: synchronous allocation).  NULL: no memory / the stream failed.
    void* get(hipStream_t st, size_t bytes, size_t slack = 0);
    void release();
private:
    struct Buf { void* p = nullptr; size_t bytes = 0; };
    const bool cleared_;
    std::mutex mu_;
    std::map<hipStream_t, Buf> bufs_;
};

// walk.hip: walk[g] = the n[g] query indices of cloud g sorted by the 12-bit Morton key of their cell in a 16^3 grid over
// the cloud's bounding box (a permutation; the order inside a cell is arbitrary), for up to four clouds in one launch.
// The gather kernels visit their queries in that order, an eighth of it per XCD.  key (or key[g]) may be NULL.
int query_walk_multi(const float* const* pts, const int* n, int* const* walk, int* const* key, int count, hipStream_t st);

// InstanceNorm + LeakyReLU from fp64 column sums for up to four tensors of one width in one launch (pointops.hip)
struct NormJob {
    const float* x; const double* sums; const float* res; const double* res_sums; float* y;
    const float* s_pts; float4* pk;      // pack form only: the KPConv support records of the output rows
    int n; double count;
    float* stats_out = nullptr;          // optional: receives the (mean, rstd) pairs [c][2] the sums stand for (the train tape keeps them)
};
int instnorm_apply_sums_multi(const NormJob* jobs, int count, int c, int ldx, float eps, int ldr, float slope, int ldy, bool pack,
                              hipStream_t st);
// the widths and leading dimensions that kernel serves (ldr = 0: no residual); 16-byte aligned bases are the caller's to check
bool instnorm_sums_ok(int c, int ldx, int ldy, int ldr = 0);

struct GatherJob { const float* x; const int64_t* idx; float* out; int ns, nq, h, ld_idx; const int* walk = nullptr; };   // walk: see query_walk_multi
int gather_max_multi(const GatherJob* jobs, int count, int c, hipStream_t st);
// closest_pool for up to four clouds of one width in ONE launch: out_g[q, :c] = x_g[idx_g[q * ld_idx], :c], a zero row for a
// first index outside [0, ns_g); x rows have leading dimension ld_x, out rows ld_out (columns c .. ld_out - 1 are not written)
struct FirstJob { const float* x; const int64_t* idx; float* out; int ns, nq, ld_idx; };
int gather_first_multi(const FirstJob* jobs, int count, int c, int ld_x, int ld_out, hipStream_t st);
int heads_multi(const float* const* x, const int* rows, int count, int ld, int fd, float* const* feats, float* const* s_ov,
                float* const* s_sal, hipStream_t st);
int copy2d_multi(const float* const* src, float* const* dst, const int* rows, int count, int ld_src, int ld_dst, int cols,
                 hipStream_t st);
int instnorm_colsums_multi(const float* const* x, double* const* sums, const int* n, int count, int c, int ldx, hipStream_t st);

// DGCNN edge convolution (gnn.hip): emax + InstanceNorm2d statistics of up to four clouds in one launch (k_edgeconv_rows)
struct EdgeCloud {
    const float* ctr; const float* nbr; const int* idx; float* emax; double* sums; int n, k;
};
bool edgeconv_rows_ok(const EdgeCloud* cl, int count, int ld_ctr, int ld_nbr, int ld_emax, int c);
int edgeconv_rows_multi(const EdgeCloud* cl, int count, int ld_ctr, int ld_nbr, int ld_emax, int c, bool atomic, int* nchunks_out,
                        hipStream_t st);

// multi-head attention on the fp32 matrix cores (gnn.hip): up to four clouds in one launch (k_attention_mfma)
struct AttnCloud { const float* q; const float* k; const float* v; float* out; int n, ms; };
bool attention_mfma_ok(const AttnCloud* cl, int count, int ldq, int ldk, int ldv, int d);
int attention_mfma_multi(const AttnCloud* cl, int count, int ldq, int ldk, int ldv, int ldo, int heads, int d, float scale,
                         hipStream_t st);
// its backward (train step): gradients ADDED to dq / dk / dv by float atomics; false: keys beyond what the score tile of a
// 32-query workgroup holds in LDS (1216), head widths other than 32 / 64 / 128, deterministic=1
bool attention_bwd_mfma_ok(int n, int ms, int d, int ldq, int ldk, int ldv, int ld_do);
int attention_bwd_mfma(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* o, int ldo,
                       const float* d_o, int ld_do, float* dq, int ld_dq, float* dk, int ld_dk, float* dv, int ld_dv, int n, int ms,
                       int heads, int d, float scale, hipStream_t st);

// Tuning / A-B switches of the library, in ONE place.  Every field defaults to the product behaviour; they are set by
// pcrcg_debug_set("name=value,name=value") or, once at first use, from the environment variable PCRCG_DEBUG (same
// syntax) -- include/pcrcg.h lists the names.  Nothing else in csrc/ reads the environment, except PCRCG_GEMM_MODE
// (the documented arithmetic selector, pcrcg_gemm_set_mode).
struct DebugOpts {
    int stat_sums = 1;         // runner: InstanceNorm statistics as fp64 column sums added by the GEMM epilogues
    int stat_sums_rows = 1 << 30;   //   ... only for outputs of up to that many rows (above: deterministic partials)
    int att_mfma = 1;          // attention: the fp32-MFMA kernel, all clouds of a call in one launch (0: the VALU kernel per cloud)
    int radius_blocks = 0;     // radius search grid (0: 512 workgroups)
    int kd_blocks = 0;
    int att_tq = 16;           // attention kernel: queries per workgroup (8 or 16)
    int kd_spin_limit = 0;     // KD-forest task queue: spin bound (0: default)
    int gemm_log = 0;          // print every GEMM's shape and grid
    int x6_tile = -1, x6_splitk = 0, x6_t1 = 1, x6_t2 = 1, x6_order = -1, x6_big = 0, x6_h2 = 1;   // split-bf16 GEMM plan overrides
    int train_side_stream = 1; // train-step backward: weight-gradient products on a second stream
    int gemm_tile = -1, gemm_splitk = 0, gemm_split_target = 768;        // fp32-MFMA GEMM plan overrides
    // deterministic=1: results that are a function of the inputs alone, bit for bit, run after run -- no floating-point
    // atomics anywhere on the path: split-K products store their partial tiles and add them in split order (a second pass,
    // gemm_x6.hip; the fp32-MFMA kernel does not split: gemm_splitk = 1), InstanceNorm statistics come from stored partials
    // and a fixed-order finishing pass (stat_sums = 0), and the train step's scatter kernels accumulate in 64-bit fixed
    // point (integer addition is associative; trainops.hip).  The 2-D backbone's BatchNorm sums are stored per row tile
    // and added by a fixed-order pass as well (conv2d.hip).  Slower (DESIGN.md has the price); the default keeps the
    // atomics.  Setting it overrides the two switches it implies.
    int deterministic = 0;
    int bwd_mfma = 1;               // KPConv backward's scatter on the matrix cores (k_kpconv_bwd_dx_mfma); 0: the VALU kernel
    // forward runner: gather launches visit their queries in XCD-local Morton order (walk.hip) where runner.hip's walk_pays()
    // says it wins; 0: index order everywhere (the order before the walk existed), 2: every launch walks (tests, A/B timing)
    int walk = 1;
};
const DebugOpts& debug_opts();

// prof.hip.  Optional start / stop events of a KPConv kernel (bench.py roofline); see pcrcg_profile_kpconv in
// include/pcrcg.h.  The events are handed to hipExtLaunchKernelGGL, so they stamp the kernel's own begin and
// end (what rocprofv3 reports), not the time its dispatch waited behind other streams.  a/b are NULL when
// profiling is off (a plain launch).  kind 0 = gather/aggregate kernel, 1 = fused kernel, 2 = bf16-storage gather kernel,
// 3 = a GEMM of the k_gemm_x6 family (nq = M, h = N, cin = K, cout = bf16 products per element: 6, or 3 with a bf16 A),
// 4 = a radius search (nq = queries, h = columns, cin = supports, cout = 1 cell-cooperative kernel / 0 per-query kernel);
// pcrcg_profile_kpconv(flags): 1 = KPConv kernels, 2 = GEMMs, 4 = radius searches.
struct KpProfScope {
    hipStream_t st;
    hipEvent_t a, b;
    int nq, h, cin, cout, kind;
    bool on;
    KpProfScope(hipStream_t s, int nq, int h, int cin, int cout, int kind);
    ~KpProfScope();
};

}  // namespace pcrcg

#define PCRCG_CHECK_ARG(cond)                                                        \
    do {                                                                             \
        if (!(cond)) {                                                               \
            pcrcg::set_error("%s: bad argument: %s", __func__, #cond);               \
            return PCRCG_EBADARG;                                                    \
        }                                                                            \
    } while (0)

#define PCRCG_CHECK_WS(carver)                                                                     \
    do {                                                                                           \
        if (!(carver).ok()) {                                                                      \
            pcrcg::set_error("%s: workspace too small (%zu needed, %zu given)", __func__,          \
                             (carver).off, (carver).cap);                                          \
            return PCRCG_EWORKSPACE;                                                               \
        }                                                                                          \
    } while (0)

#define PCRCG_CHECK_HIP(expr)                                                                  \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) {                                                                \
            pcrcg::set_error("%s: %s failed: %s", __func__, #expr, hipGetErrorString(e_));     \
            return PCRCG_ELAUNCH;                                                              \
        }                                                                                      \
    } while (0)

#define PCRCG_CHECK_LAUNCH() PCRCG_CHECK_HIP(hipGetLastError())

// A kernel that may ask for more than 64 KB of dynamic LDS is granted, ONCE per kernel and under std::call_once, everything a
// gfx950 workgroup can have (160 KB minus the kernel's static LDS).  The grant only lifts the launch-time limit -- what a
// launch allocates is its own `lds` argument -- and it never shrinks, so host threads that launch the same kernel with
// different sizes (the pair engine's model threads) cannot undo one another's setting.
namespace pcrcg {
inline hipError_t grant_max_dyn_lds(const void* kern) {
    hipFuncAttributes at;
    hipError_t e = hipFuncGetAttributes(&at, kern);
    if (e != hipSuccess) return e;
    const int cap = 160 * 1024 - (int)at.sharedSizeBytes;
    return hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, cap);
}
}  // namespace pcrcg
#define PCRCG_GRANT_LDS(kern)                                                                                   \
    do {                                                                                                        \
        static std::once_flag once_;                                                                            \
        static hipError_t granted_ = hipSuccess;                                                                \
        std::call_once(once_, [&] { granted_ = pcrcg::grant_max_dyn_lds(reinterpret_cast<const void*>(kern)); }); \
        PCRCG_CHECK_HIP(granted_);                                                                              \
    } while (0)

#define PCRCG_PROPAGATE(expr)      \
    do {                           \
        int rc_ = (expr);          \
        if (rc_ != PCRCG_OK) return rc_; \
    } while (0)
