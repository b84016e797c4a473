// runner.hip -- host-side network runner: enqueues the whole KPFCNN forward
// (ref:models/architectures.py:181-191, 516-610; blocks ref:models/blocks.py:536-709; GNN
// ref:models/gcn.py:96-217) from ONE C-ABI call.  It contains no device code of its own: it sequences
// the kernels of this library (pcrcg_* entry points) over a caller-provided arena, exactly like the
// Python mirror in pcrcg_amd/{blocks,gcn,architectures}.py does op by op -- the two are compared in
// tests/test_model_gpu.py.  The point is host cost: several hundred kernel launches per fragment pair
// cost one FFI crossing instead of several hundred.
//
// Memory: block outputs live until the end of the forward (skip connections need some of them and the
// total is ~0.25 GB for a 2 x 30k-point pair); temporaries of a block are released when it returns
// (stack discipline).  pcrcg_kpfcnn_ws_bytes runs the same code with launches disabled to size it.
#include <vector>

#include <cstdlib>

#include "gemm.h"
#include "kpconv.h"

namespace pcrcg {
namespace {

constexpr int GMAX = 4;   // fragment pairs one call can carry (pcrcg_kpfcnn_forward_group)
// c.G <= GMAX everywhere below (validate_group; the two stacking sites double it only while 2 * c.G <= GMAX), and every
// multi-cloud kernel of common.h takes that many: all clouds of a call always fit ONE launch of them, no per-cloud loop for the
// count's sake.  The per-cloud paths that remain are for what those kernels refuse (alignment, widths, arithmetic mode).
static_assert(GMAX <= 4, "instnorm_apply_sums_multi, instnorm_colsums_multi, gather_max_multi, gather_first_multi, copy2d_multi, heads_multi, "
                         "edgeconv_rows_multi and attention_mfma_multi (common.h) take up to four clouds");

// Row-major fp32 matrix view -- one per fragment pair of the call (same width and leading dimension, own rows).  With
// several pairs every operator below runs its per-pair kernels once per pair and its weight products ONCE for all pairs (GemmGroup):
// the pairs never mix (InstanceNorm statistics, neighbour tables, kNN and attention stay per pair -- SURVEY.md 8e), but a
// coarse-level product that fills a fifth of the chip for one pair fills twice that for two at the same duration, and
// every product costs one launch per two pairs.
struct Mat {
    float* p[GMAX] = {};
    int rows[GMAX] = {};
    int cols = 0, ld = 0;
    bool zeroed = false;   // lives in the zero arena and has not been written yet
};

struct Ctx {
    char* base = nullptr;
    size_t cap = 0, off = 0, peak = 0;
    hipStream_t st = nullptr;
    bool dry = false;
    bool bf16 = false;      // pcrcg_model.feature_bf16
    int G = 1;              // pairs of this call
    int rc = PCRCG_OK;

    void* raw(size_t bytes) {
        bytes = (bytes + 255) & ~size_t(255);
        void* p = base ? base + off : nullptr;
        off += bytes;
        if (off > peak) peak = off;
        if (!dry && off > cap && rc == PCRCG_OK) {
            set_error("pcrcg_kpfcnn_forward: workspace too small (%zu needed so far, %zu given)", off, cap);
            rc = PCRCG_EWORKSPACE;
        }
        return p;
    }
    Mat mat(const int* rows, int cols, int ld = 0) {
        Mat m;
        m.cols = cols; m.ld = ld ? ld : cols;
        for (int g = 0; g < G; ++g) {
            m.rows[g] = rows[g];
            m.p[g] = static_cast<float*>(raw((size_t)(rows[g] > 0 ? rows[g] : 1) * m.ld * sizeof(float)));
        }
        return m;
    }
    // Zero arena: the front part of the workspace, cleared by ONE memset at the start of the forward and handed out
    // without reuse.  Outputs of split-K products come from it (the product accumulates into C with atomics and would
    // otherwise clear C itself: 39 memset launches per S30k forward).
    char* zbase = nullptr;
    size_t zcap = 0, zoff = 0;
    void* zraw(size_t bytes) {
        bytes = (bytes + 255) & ~size_t(255);
        void* p = zbase ? zbase + zoff : nullptr;
        zoff += bytes;
        if (!dry && zoff > zcap && rc == PCRCG_OK) {
            set_error("pcrcg_kpfcnn_forward: zero arena too small (%zu needed so far, %zu reserved)", zoff, zcap);
            rc = PCRCG_EWORKSPACE;
        }
        return p;
    }
    int max_rows(const int* rows) const { int m = rows[0]; for (int g = 1; g < G; ++g) m = rows[g] > m ? rows[g] : m; return m; }
    // the output of a [rows, k] x [cols, k]^T product (the plan of the pair with most rows decides for all)
    Mat gemm_out(const int* rows, int cols, int k, int ld = 0) {
        long total = 0;
        for (int g = 0; g < G; ++g) total += rows[g];
        if (!gemm_bt_accumulates(max_rows(rows), cols, k, total)) return mat(rows, cols, ld);
        Mat m;
        m.cols = cols; m.ld = ld ? ld : cols;
        for (int g = 0; g < G; ++g) {
            m.rows[g] = rows[g];
            m.p[g] = static_cast<float*>(zraw((size_t)(rows[g] > 0 ? rows[g] : 1) * m.ld * sizeof(float)));
        }
        m.zeroed = true;
        return m;
    }
    size_t mark() const { return off; }
    void release(size_t m) { off = m; }
    bool live() const { return !dry && rc == PCRCG_OK; }
    void check(int r) { if (r != PCRCG_OK && rc == PCRCG_OK) rc = r; }
    // several pairs in one launch: only with the split-bf16 arithmetic (PCRCG_GEMM_MODE=0 runs the products pair by pair)
    bool paired() const { return G >= 2 && gemm_split_terms_on(); }
    // a piece of the forward over twice the clouds (stacked() below); what it allocates stays allocated
    template <class F> Mat twice(F&& f) { G *= 2; const Mat r = f(); G /= 2; return r; }
};

inline int pad4(int v) { return (v + 3) & ~3; }
inline Mat cols(const Mat& m, int c0, int n) {
    Mat r = m;
    for (int g = 0; g < GMAX; ++g) r.p[g] = m.p[g] ? m.p[g] + c0 : nullptr;
    r.cols = n;
    return r;
}
// rows [r0[g], r0[g] + n[g]) of every pair's matrix
inline Mat rows(const Mat& m, const int* r0, const int* n) {
    Mat r = m;
    for (int g = 0; g < GMAX; ++g) {
        r.p[g] = m.p[g] ? m.p[g] + (long)r0[g] * m.ld : nullptr;
        r.rows[g] = n[g];
    }
    return r;
}
// The two clouds of every pair as 2 * G0 independent clouds, [a of every pair | b of every pair], and either half of such a matrix
inline Mat stacked(const Mat& a, const Mat& b, int G0) {
    Mat m = a;
    for (int g = 0; g < G0; ++g) { m.p[G0 + g] = b.p[g]; m.rows[G0 + g] = b.rows[g]; }
    return m;
}
inline Mat half(const Mat& m, int which, int G0) {
    Mat r = m;
    for (int g = 0; g < GMAX; ++g) {
        r.p[g] = g < G0 ? m.p[which * G0 + g] : nullptr;
        r.rows[g] = g < G0 ? m.rows[which * G0 + g] : 0;
    }
    return r;
}

// A GEMM output together with the InstanceNorm column partials its epilogue may have produced (per pair).
struct Stat {
    void* partials[GMAX] = {};                // [2][cols][chunks] fp64 partials; or, when `sums`, zeroed [2][cols] fp64 accumulators
    size_t bytes = 0;
    int chunks[GMAX] = {};                    // what the producer left (GemmCall::h_chunks): SUMS, NOTHING, or > 0 chunks of partials
    bool sums = false;
    static constexpr int SUMS = -1, NOTHING = 0;
    bool has_sums(int g) const { return chunks[g] == SUMS; }        // the accumulators hold the column sums
    bool nothing(int g) const { return chunks[g] == NOTHING; }
};

// The GEMM epilogue adds its output's column sums into accumulators from the zero arena with fp64 atomics -- one pair per
// column and 64-row tile, the workgroup's two row halves meet in LDS first -- and the normalisation derives mean / rstd
// from them itself: no partial buffers, no finishing launch (51 per S30k forward before).  With the per-wavefront
// atomics of the first version the 60 000-row outputs (1 876 per address) measured slower than partials + finishing
// kernel and kept those; with one per tile (938) the sums win everywhere: 470-473 vs 457-466 pairs/s.
// (DebugOpts::stat_sums_rows: outputs above that many rows keep the deterministic partials.)
Stat stat_buffer(Ctx& c, const int* rows, int cols) {
    Stat s;
    const int mr = c.max_rows(rows);
    if (debug_opts().stat_sums && mr <= debug_opts().stat_sums_rows && gemm_split_terms_on()) {
        s.sums = true;
        s.bytes = 2 * sizeof(double) * (size_t)cols;
        for (int g = 0; g < c.G; ++g) s.partials[g] = c.zraw(s.bytes);
        return s;
    }
    s.bytes = pcrcg_gemm_colstats_bytes(mr, cols);
    for (int g = 0; g < c.G; ++g) s.partials[g] = c.raw(s.bytes);
    return s;
}

// widths the sums form of the normalisation kernel serves (its thread -> channel-group map)
inline bool sums_apply_ok(const Mat& x, const Mat& y, const Mat* res) {
    return instnorm_sums_ok(x.cols, x.ld, y.ld, res ? res->ld : 0);
}

// (mean, rstd) of pair g's x: from the producing GEMM's partials when it left some, else by a pass over x
void col_stats(Ctx& c, const Mat& x, int g, const Stat* s, float* stats, void* ws, size_t wsb) {
    if (s && !s->nothing(g))          // (column sums: the finishing kernel reads them as one chunk per column)
        c.check(pcrcg_instnorm_stats_from_partials(s->partials[g], s->has_sums(g) ? 1 : s->chunks[g], x.cols, (double)x.rows[g], 1e-5f,
                                                   stats, c.st));
    else
        c.check(pcrcg_instnorm_stats(x.p[g], x.rows[g], x.cols, x.ld, 1e-5f, stats, ws, wsb, c.st));
}

// sums-mode statistics the producing product could not leave (a split-K product): one pass into the same accumulators
void fill_sums(Ctx& c, const Mat& x, Stat* xs) {
    if (!c.live() || !xs || !xs->sums) return;
    {   // the pairs whose product left nothing: one launch for all of them
        const float* xp[GMAX]; double* sp[GMAX]; int np[GMAX]; int idx[GMAX]; int cnt = 0;
        for (int g = 0; g < c.G; ++g)
            if (xs->nothing(g) && x.rows[g] >= 1) { xp[cnt] = x.p[g]; sp[cnt] = static_cast<double*>(xs->partials[g]); np[cnt] = x.rows[g]; idx[cnt++] = g; }
        if (cnt >= 2) {
            c.check(instnorm_colsums_multi(xp, sp, np, cnt, x.cols, x.ld, c.st));
            for (int i = 0; i < cnt; ++i) xs->chunks[idx[i]] = Stat::SUMS;
        }
    }
    for (int g = 0; g < c.G; ++g)
        if (xs->nothing(g)) {
            c.check(pcrcg_instnorm_colsums(x.p[g], x.rows[g], x.cols, x.ld, xs->partials[g], c.st));
            xs->chunks[g] = Stat::SUMS;
        }
}
inline bool all_sums(const Ctx& c, const Stat* s) {
    if (!s) return false;
    for (int g = 0; g < c.G; ++g)
        if (!s->has_sums(g)) return false;
    return true;
}

// The sums form of the normalisation (instnorm_apply_sums_multi) for all clouds of the call: y = lrelu(IN(x) [+ IN(res) | + res])
// with x's statistics in sums[g] (res_sums: res is normalised too).  `aligned`: every base is 16-byte aligned, which the
// kernel's float4 accesses need.  Callers with other row counts or the pack form edit the jobs.
struct NormJobs {
    NormJob j[GMAX];
    bool aligned = true;
};
NormJobs norm_jobs(const Ctx& c, const Mat& x, void* const* sums, const Mat& y, const Mat* res = nullptr, void* const* res_sums = nullptr) {
    NormJobs nj;
    for (int g = 0; g < c.G; ++g) {
        const float* r = res ? res->p[g] : nullptr;
        nj.j[g] = NormJob{x.p[g], static_cast<const double*>(sums[g]), r, res_sums ? static_cast<const double*>(res_sums[g]) : nullptr,
                          y.p[g], nullptr, nullptr, x.rows[g], (double)(x.rows[g] > 0 ? x.rows[g] : 1)};
        nj.aligned = nj.aligned && ((reinterpret_cast<uintptr_t>(x.p[g]) | reinterpret_cast<uintptr_t>(y.p[g]) | reinterpret_cast<uintptr_t>(r)) & 15) == 0;
    }
    return nj;
}
// all clouds in ONE launch (a launch per cloud cost the stream ~5 us of queue time each), else the single-tensor entry per cloud
void apply_sums(Ctx& c, const NormJob* jobs, bool one_launch, int cols, int ldx, int ldr, float slope, int ldy) {
    if (one_launch) {
        c.check(instnorm_apply_sums_multi(jobs, c.G, cols, ldx, 1e-5f, ldr, slope, ldy, false, c.st));
        return;
    }
    for (int g = 0; g < c.G; ++g) {
        const NormJob& j = jobs[g];
        c.check(pcrcg_instnorm_apply_sums(j.x, j.n, cols, ldx, j.sums, j.count, 1e-5f, j.res, ldr, j.res_sums, slope, j.y, ldy, c.st));
    }
}

// y = lrelu(IN(x) [+ IN(res) | + res], slope)
void norm_act(Ctx& c, const Mat& x, float slope, const Mat& y, Stat* xs = nullptr, const Mat* res = nullptr,
              bool norm_res = false, Stat* rs = nullptr) {
    fill_sums(c, x, xs);
    if (res && norm_res) fill_sums(c, *res, rs);
    if (c.live() && all_sums(c, xs) && (!res || !norm_res || all_sums(c, rs)) && sums_apply_ok(x, y, res)) {
        const NormJobs nj = norm_jobs(c, x, xs->partials, y, res, (res && norm_res) ? rs->partials : nullptr);
        apply_sums(c, nj.j, nj.aligned, x.cols, x.ld, res ? res->ld : 0, slope, y.ld);
        return;
    }
    const size_t m = c.mark();
    float* stats = static_cast<float*>(c.raw(sizeof(float) * 2 * x.cols));
    float* rstats = (res && norm_res) ? static_cast<float*>(c.raw(sizeof(float) * 2 * x.cols)) : nullptr;
    const size_t wsb = pcrcg_instnorm_ws_bytes(x.cols);
    void* ws = c.raw(wsb);
    if (c.live())
        for (int g = 0; g < c.G; ++g) {
            col_stats(c, x, g, xs, stats, ws, wsb);
            if (rstats) col_stats(c, *res, g, rs, rstats, ws, wsb);
            c.check(pcrcg_instnorm_apply(x.p[g], x.rows[g], x.cols, x.ld, stats, res ? res->p[g] : nullptr, res ? res->ld : 0,
                                         rstats, slope, y.p[g], y.ld, c.st));
        }
    c.release(m);
}

// where pair g's product leaves the column statistics of its output
void stats_into(GemmCall& call, Stat* st, int g) {
    if (!st) return;
    call.colstats = st->partials[g];
    call.colstats_bytes = st->bytes;
    call.h_chunks = &st->chunks[g];
    call.colstats_sums = st->sums;
}
// What a product may fold into its A loads, for all pairs.  sums: per-pair column sums of the raw A (normalise-on-load), or NULL
struct Fold {
    Stat* sums = nullptr;
    float slope = 1.0f;
    bool accumulate = false;
};
GemmExtra extra_of(const Fold& f, const Mat& x, int g) {
    GemmExtra ex;
    if (f.sums) {
        ex.a_sums = static_cast<const double*>(f.sums->partials[g]);
        ex.a_count = (double)x.rows[g];
        ex.a_slope = f.slope;
    }
    ex.accumulate = f.accumulate;
    return ex;
}
// the further pairs' sides of a product
GemmGroup group_of(const Ctx& c, const Mat& x, const Mat& y, bool c_zeroed, Stat* st, const float* const* row_scale, const Fold* f) {
    GemmGroup grp;
    grp.n = c.G - 1;
    for (int g = 1; g < c.G; ++g) {
        GemmPair& p = grp.p[g - 1];
        p.a = x.p[g];
        p.c = y.p[g];
        p.m = x.rows[g];
        p.row_scale = row_scale ? row_scale[g] : nullptr;
        p.colstats = st ? st->partials[g] : nullptr;
        p.h_chunks = st ? &st->chunks[g] : nullptr;
        p.c_zeroed = c_zeroed;
        if (f && f->sums) { p.a_sums = static_cast<const double*>(f->sums->partials[g]); p.a_count = (double)x.rows[g]; }
    }
    return grp;
}

// y (+)= f(x)[rows] @ w^T (+ bias); w is [out, in] with leading dimension ldw; optionally leaves the column statistics of y
// for the InstanceNorm that follows.  row_scale: per-pair row factors (KPConv's 1 / neighbour count); f: the GemmExtra
// forms (NULL: a plain product, which also runs without the split-term arithmetic); c_zeroed: y is known to be all zeros.
// All pairs in one launch when they can share it.
void linear(Ctx& c, const Mat& x, const float* w, int ldw, const float* bias, const Mat& y, bool c_zeroed, Stat* st = nullptr,
            const float* const* row_scale = nullptr, const Fold* f = nullptr) {
    if (!c.live()) return;
    const bool grouped = c.paired();
    for (int g = 0; g < (grouped ? 1 : c.G); ++g) {
        GemmCall call;
        call.a = x.p[g]; call.lda = x.ld;
        call.b = w; call.ldb = ldw;
        call.c = y.p[g]; call.ldc = y.ld;
        call.m = x.rows[g]; call.n = y.cols; call.k = x.cols;
        call.row_scale = row_scale ? row_scale[g] : nullptr;
        call.bias = bias;
        call.st = c.st;
        stats_into(call, st, g);
        call.c_zeroed = c_zeroed;
        const GemmExtra ex = f ? extra_of(*f, x, g) : GemmExtra();
        const GemmGroup grp = grouped ? group_of(c, x, y, c_zeroed, st, row_scale, f) : GemmGroup();
        if (f) call.ex = &ex;
        if (grouped) call.grp = &grp;
        c.check(gemm_run(call));
    }
}
void linear(Ctx& c, const Mat& x, const float* w, int ldw, const float* bias, const Mat& y, Stat* st = nullptr,
            const float* const* row_scale = nullptr) {
    linear(c, x, w, ldw, bias, y, y.zeroed, st, row_scale);
}

// y = lrelu(IN(x), slope) @ w^T (+ bias) with the normalisation done inside the product's A loads (GemmExtra::a_sums):
// x is the RAW output of the producing product and xs its column sums.  Returns false when that form does not apply
// (the caller then normalises into a matrix of its own and calls linear()).
bool lazy_stats_ready(Ctx& c, const Mat& x, Stat* xs) {
    if (!xs || !xs->sums || x.ld % 4 != 0 || x.cols > 4096) return false;
    fill_sums(c, x, xs);              // nobody left the sums yet (split-K or accumulated output): one pass
    return true;
}
bool linear_norm(Ctx& c, const Mat& x, Stat* xs, float slope, const float* w, int ldw, const float* bias, const Mat& y,
                 Stat* st = nullptr) {
    if (!gemm_split_terms_on() || !lazy_stats_ready(c, x, xs)) return false;
    Fold f;
    f.sums = xs;
    f.slope = slope;
    linear(c, x, w, ldw, bias, y, y.zeroed, st, nullptr, &f);
    return true;
}

struct Batches { const pcrcg_batch* b[GMAX]; };

// The gather launches' query order (walk.hip): one walk per level and pair, shared by every launch whose QUERIES are that
// level's points -- the level's own KPConvs, the strided KPConv of the level above and its max-pool.  forward() takes the
// memory before the blocks (it lives until the call ends); the walk kernel of a level runs when the first launch asks.
struct Walks {
    int* w[PCRCG_MAX_LEVELS][GMAX] = {};
    bool built[PCRCG_MAX_LEVELS] = {};
    int mode = 0;      // DebugOpts::walk as forward() read it ONCE: the buffers above exist iff mode != 0, whatever the switch does later
};

// Which launches walk: those whose support feature rows ([ns, cin] fp32) exceed 8 MB, two XCDs' L2s, and that have at least
// 2048 queries.  From the fourteen gather and pool launches of one S30k pair timed alone with and without the walk
// (profiles/walk_ab.txt): the 15 MB to 61 MB launches gain 5 % to 50 %; at 7.9 MB two of three launches LOSE 4-5 % and at
// 4 MB and below nothing moves (every L2 holds most rows whatever the order, the walk only adds its index load); the
// level-2 pool (16 MB, 763 queries) saves less than the walk kernel of its level costs.
static bool walk_pays(int mode, int ns, int cin, int nq) {
    if (mode != 1) return mode == 2;
    return (size_t)ns * (size_t)cin * sizeof(float) > (size_t)8 << 20 && nq >= 2048;
}

// the walks of level l's points for every pair of the call (NULL entries while sizing)
const int* const* level_walks(Ctx& c, const Batches& B, Walks& W, int l) {
    if (c.live() && !W.built[l]) {
        const float* pts[GMAX];
        int n[GMAX];
        for (int g = 0; g < c.G; ++g) { pts[g] = B.b[g]->points[l]; n[g] = B.b[g]->n_points[l]; }
        c.check(query_walk_multi(pts, n, W.w[l], nullptr, c.G, c.st));
        W.built[l] = true;
    }
    return W.w[l];
}

// input channels of the block's KPConv as the gather kernel sees them (padded to a multiple of 4)
int kp_cin(const pcrcg_block& blk, const Mat& x) { return (blk.kp_w_pad && blk.cin_pad > x.cols) ? blk.cin_pad : x.cols; }
// the k-major weights [15 * kp_cin, cout] that match those channels: the zero-padded copy whenever the gather sees cin_pad
// of them -- features padded by kpconv() below (x.cols < cin_pad) or handed over padded by the caller (x.cols == cin_pad)
const float* kp_weight(const pcrcg_block& blk, const Mat& x) {
    return (blk.kp_w_pad && blk.cin_pad > 0 && kp_cin(blk, x) == blk.cin_pad) ? blk.kp_w_pad : blk.kp_w;
}

// length of a wf row (the contraction's K).  cin = 1 (the first layer of the geometry-only configurations) with a K-contiguous
// weight copy: that copy has rows of 16 floats (the 16th zero, pcrcg_amd/runner.py) and the gather kernel writes wf in rows of
// 16 -- whole k-steps, so the contraction is the grouped fp16 A B^T product with the statistics in its epilogue like every other
// layer's (round 6; before: one k-major six-product launch per pair and a column-sum pass over its output)
int kp_k(const pcrcg_block& blk, const Mat& x) {
    const int cin = kp_cin(blk, x);
    return (cin == 1 && blk.kp_wt) ? 16 : PCRCG_KPOINTS * cin;
}

void kpconv(Ctx& c, const Batches& B, Walks& W, const pcrcg_block& blk, const Mat& x, const Mat& y, Stat* st = nullptr,
            void* const* packed_ws = nullptr) {
    const int l = blk.layer;
    const size_t m = c.mark();
    // channel counts that are not a multiple of 4 (the 129-channel PCR-CG input): zero-padded copy of the
    // features + zero-padded weights, so that the MFMA gather kernel applies (zeros change neither the sums nor
    // the neighbour count of the normaliser)
    Mat xin = x;
    const float* const w = kp_weight(blk, x);
    const int cin = kp_cin(blk, x);
    if (cin > x.cols) {
        xin = c.mat(x.rows, cin);
        if (c.live())
            for (int g = 0; g < c.G; ++g) {
                c.check(hipMemsetAsync(xin.p[g], 0, sizeof(float) * (size_t)x.rows[g] * cin, c.st) == hipSuccess ? PCRCG_OK
                                                                                                                   : PCRCG_ELAUNCH);
                c.check(pcrcg_copy2d(x.p[g], x.ld, xin.p[g], cin, x.rows[g], x.cols, c.st));
            }
    }
    int nq[GMAX], ns[GMAX];
    const float* q[GMAX];
    const pcrcg_table* tab[GMAX];
    float* inv_n[GMAX];
    void* ws[GMAX];
    size_t wsb[GMAX];
    for (int g = 0; g < c.G; ++g) {
        const pcrcg_batch& b = *B.b[g];
        tab[g] = blk.strided ? &b.pools[l] : &b.neighbors[l];
        q[g] = blk.strided ? b.points[l + 1] : b.points[l];
        nq[g] = blk.strided ? b.n_points[l + 1] : b.n_points[l];
        ns[g] = b.n_points[l];
        inv_n[g] = static_cast<float*>(c.raw(sizeof(float) * (nq[g] > 0 ? nq[g] : 1)));
        wsb[g] = pcrcg_kpconv_ws_bytes(ns[g]);
        ws[g] = (packed_ws && packed_ws[g]) ? packed_ws[g] : c.raw(wsb[g]);
    }
    const float* const kp_wt = blk.kp_wt;     // (cin = 1: the copy is the 16-float form or nothing)
    const int kk = kp_k(blk, x);
    // the queries' order: the walk of the level the QUERIES are points of (cin = 1 reads only the support records: no walk)
    const int* const* walks = (cin > 1 && walk_pays(W.mode, c.max_rows(ns), cin, c.max_rows(nq))) ? level_walks(c, B, W, blk.strided ? l + 1 : l) : nullptr;
    auto gather_call = [&](int g) {
        KpconvCall k;
        k.q_pts = q[g]; k.nq = nq[g]; k.s_pts = B.b[g]->points[l]; k.ns = ns[g];
        k.idx = tab[g]->idx; k.h = tab[g]->cols; k.ld_idx = tab[g]->ld;
        k.x = xin.p[g]; k.cin = cin; k.kp = blk.kp; k.extent = blk.extent;
        k.inv_n = inv_n[g]; k.ws = ws[g]; k.ws_bytes = wsb[g]; k.st = c.st;
        k.walk = walks ? walks[g] : nullptr;
        return k;
    };
    // bf16 feature storage (pcrcg_model.feature_bf16): the gathers read a bf16 copy of x and wf is bf16 in HBM -- half
    // the bytes of the two streams that bound the encoder; the contraction takes wf as the (single-term) bf16 operand
    // against the exact three-term split of the fp32 weights, fp32 accumulate and fp32 output.
    if (c.bf16 && kp_wt && cin % 32 == 0) {
        for (int g = 0; g < c.G; ++g) {
            void* xb = c.raw(sizeof(unsigned short) * (size_t)(ns[g] > 0 ? ns[g] : 1) * cin);
            void* wfb = c.raw(sizeof(unsigned short) * (size_t)(nq[g] > 0 ? nq[g] : 1) * kk);
            if (c.live()) {
                KpconvCall gather_bf16 = gather_call(g);
                gather_bf16.form = KpForm::bf16;
                gather_bf16.x_bf16 = static_cast<unsigned short*>(xb);
                gather_bf16.wf_bf16 = static_cast<unsigned short*>(wfb);
                c.check(kpconv_run(gather_bf16));
                GemmCall call;
                call.a = wfb; call.lda = kk; call.a_form = GemmA::row_bf16;
                call.b = kp_wt; call.ldb = kk;
                call.c = y.p[g]; call.ldc = y.ld;
                call.m = nq[g]; call.n = y.cols; call.k = kk;
                call.row_scale = inv_n[g];
                call.c_zeroed = y.zeroed;
                call.st = c.st;
                stats_into(call, st, g);
                c.check(gemm_run(call));
            }
        }
        c.release(m);
        return;
    }
    // cin = 1 with column-sum statistics: gather, contraction, row scale and the sums in one kernel per cloud -- no wf matrix
    // and no K = 16 product.  (stat_sums=0, deterministic=1, PCRCG_GEMM_MODE=0, a descriptor without kp_wt and widths
    // the kernel does not serve keep the two launches below.)
    if (cin == 1 && st && st->sums && kpconv_c1_fused_ok(y.cols, kp_wt)) {
        if (c.live())
            for (int g = 0; g < c.G; ++g) {
                KpconvCall layer = gather_call(g);
                layer.form = KpForm::c1_fused;
                layer.wt = kp_wt; layer.cout = y.cols; layer.y = y.p[g]; layer.ld_y = y.ld;
                layer.sums = static_cast<double*>(st->partials[g]);
                c.check(kpconv_run(layer));
                st->chunks[g] = Stat::SUMS;
            }
        c.release(m);
        return;
    }
    Mat wf = c.mat(nq, kk);
    if (c.live()) {
        for (int g = 0; g < c.G; ++g) {
            // (pcrcg_kpconv_aggregate is this call with pack = true; the support records are there already when the
            // normalisation that wrote x packed them, norm_act_pack)
            KpconvCall gather = gather_call(g);
            gather.wf = wf.p[g];
            gather.pack = !(kk != 16 && packed_ws && packed_ws[g] && xin.p[g] == x.p[g]);
            gather.c1_ld = kk == 16 ? 16 : 0;
            c.check(kpconv_run(gather));
        }
        // contraction wf @ W: against the K-contiguous copy wt [cout, 15*cin] when the descriptor carries one
        // (C = A * B^T form: both operands k-contiguous, the form the split-bf16 GEMM is built for).
        // (Measured and not adopted, rounds 2 and 3: aggregating + contracting row chunks so that wf stays in L2 /
        // Infinity Cache between the two kernels -- isolated 3.50 vs 3.31 ms per forward with 48 MB chunks; inside the
        // engine 416 / 446 / 459 / 462 pairs/s with 16 / 32 / 64 / 120 MB chunks against 460-464 unchunked: the extra
        // launches cost more than the on-chip re-read saves.)
        if (kp_wt)
            linear(c, wf, kp_wt, kk, nullptr, y, st, inv_n);
        else   // (descriptor without the K-contiguous weight copy: the plain entry point knows only the partials layout)
            for (int g = 0; g < c.G; ++g)
                c.check(pcrcg_gemm_f32_colstats(wf.p[g], wf.ld, w, y.cols, 0, y.p[g], y.ld, nq[g], y.cols, kk, inv_n[g], nullptr,
                                                (st && !st->sums) ? st->partials[g] : nullptr, (st && !st->sums) ? st->bytes : 0,
                                                (st && !st->sums) ? &st->chunks[g] : nullptr, c.st));
    }
    c.release(m);
}

void out_rows(const Ctx& c, const Batches& B, const pcrcg_block& blk, int* rows) {
    for (int g = 0; g < GMAX; ++g)
        rows[g] = g < c.G ? (blk.strided ? B.b[g]->n_points[blk.layer + 1] : B.b[g]->n_points[blk.layer]) : 0;
}

// SimpleBlock.forward (ref:models/blocks.py:578-590)
Mat simple_block(Ctx& c, const Batches& B, Walks& W, const pcrcg_block& blk, const Mat& x) {
    int nq[GMAX];
    out_rows(c, B, blk, nq);
    Mat y = c.mat(nq, blk.mid_dim);
    const size_t m = c.mark();
    Mat t = c.gemm_out(nq, y.cols, kp_k(blk, x));
    Stat ts = stat_buffer(c, nq, t.cols);
    kpconv(c, B, W, blk, x, t, &ts);
    norm_act(c, t, 0.1f, y, &ts);
    c.release(m);
    return y;
}

// u = lrelu(IN(t), slope) for a u that is the input of the block's KPConv: the normalisation kernel leaves the KPConv's
// support records (coordinates + "feature row sums to a positive value" flag) in kp_ws as it goes, so the KPConv needs no
// pass over u of its own (10 launches per S30k forward: +4 % pairs/s with them knocked out).  False: not applicable.
bool norm_act_pack(Ctx& c, const Batches& B, int layer, const Mat& t, float slope, const Mat& u, Stat* ts, void* const* kp_ws,
                   const size_t* kp_ws_bytes) {
    if (c.bf16 || !instnorm_pack_ok(t.cols, t.ld, u.ld) || u.ld != u.cols) return false;
    const size_t m = c.mark();
    float* stats = static_cast<float*>(c.raw(sizeof(float) * 2 * t.cols));
    const size_t wsb = pcrcg_instnorm_ws_bytes(t.cols);
    void* ws = c.raw(wsb);
    fill_sums(c, t, ts);              // a split-K product left nothing: one pass into the accumulators
    if (c.live() && all_sums(c, ts)) {          // every pair of the call in one launch
        NormJobs nj = norm_jobs(c, t, ts->partials, u);
        bool ok = nj.aligned;
        for (int g = 0; g < c.G; ++g) {
            nj.j[g].s_pts = B.b[g]->points[layer];
            nj.j[g].pk = kpconv_pk_ptr(kp_ws[g], kp_ws_bytes[g], t.rows[g]);
            ok = ok && nj.j[g].pk != nullptr;
        }
        if (ok) {
            c.check(instnorm_apply_sums_multi(nj.j, c.G, t.cols, t.ld, 1e-5f, 0, slope, u.ld, true, c.st));
            c.release(m);
            return true;
        }
    }
    if (c.live())
        for (int g = 0; g < c.G; ++g) {
            const float* s_pts = B.b[g]->points[layer];
            float4* pk = kpconv_pk_ptr(kp_ws[g], kp_ws_bytes[g], t.rows[g]);
            if (!pk) c.check(PCRCG_EWORKSPACE);
            else if (ts && ts->has_sums(g))
                c.check(instnorm_apply_pack(t.p[g], t.rows[g], t.cols, t.ld, nullptr, static_cast<const double*>(ts->partials[g]),
                                            (double)t.rows[g], 1e-5f, slope, u.p[g], u.ld, s_pts, pk, c.st));
            else {
                col_stats(c, t, g, ts, stats, ws, wsb);
                c.check(instnorm_apply_pack(t.p[g], t.rows[g], t.cols, t.ld, stats, nullptr, 0.0, 1e-5f, slope, u.p[g], u.ld, s_pts,
                                            pk, c.st));
            }
        }
    c.release(m);
    return true;
}

// ResnetBottleneckBlock.forward (ref:models/blocks.py:650-678)
Mat resnet_block(Ctx& c, const Batches& B, Walks& W, const pcrcg_block& blk, const Mat& feats) {
    int nq[GMAX];
    out_rows(c, B, blk, nq);
    Mat y = c.mat(nq, blk.out_dim);
    const size_t m = c.mark();
    Mat x = feats;
    void* kp_ws[GMAX] = {};
    size_t kp_wsb[GMAX] = {};
    bool packed = false;
    if (blk.unary1) {
        Mat t = c.gemm_out(feats.rows, blk.mid_dim, feats.cols), u = c.mat(feats.rows, blk.mid_dim);
        Stat ts = stat_buffer(c, t.rows, t.cols);
        linear(c, feats, blk.unary1, feats.cols, nullptr, t, &ts);
        // u feeds the KPConv whose supports are this block's input rows: pack its support records on the way
        if (blk.mid_dim % 4 == 0 && !(blk.kp_w_pad && blk.cin_pad > blk.mid_dim)) {
            for (int g = 0; g < c.G; ++g) {
                kp_wsb[g] = pcrcg_kpconv_ws_bytes(feats.rows[g]);
                kp_ws[g] = c.raw(kp_wsb[g]);
            }
            packed = norm_act_pack(c, B, blk.layer, t, 0.1f, u, &ts, kp_ws, kp_wsb);
        }
        if (!packed) norm_act(c, t, 0.1f, u, &ts);
        x = u;
    }
    Mat k = c.gemm_out(nq, blk.mid_dim, PCRCG_KPOINTS * kp_cin(blk, x)), kn = c.mat(nq, blk.mid_dim);
    Stat ks = stat_buffer(c, nq, blk.mid_dim);
    kpconv(c, B, W, blk, x, k, &ks, packed ? kp_ws : nullptr);
    Mat u2 = c.gemm_out(nq, blk.out_dim, blk.mid_dim);
    Stat u2s = stat_buffer(c, nq, blk.out_dim);
    // lrelu(IN(k)) is read by unary2 alone: its product normalises k on load when k's statistics are column sums
    if (!linear_norm(c, k, &ks, 0.1f, blk.unary2, blk.mid_dim, nullptr, u2, &u2s)) {
        norm_act(c, k, 0.1f, kn, &ks);
        linear(c, kn, blk.unary2, blk.mid_dim, nullptr, u2, &u2s);
    }
    Mat sc = feats;
    if (blk.strided) {   // max_pool shortcut (:672-673)
        sc = c.mat(nq, feats.cols);
        if (c.live()) {          // every pair's pool in one launch
            GatherJob jobs[GMAX];
            // (its queries are level layer + 1's points: their walk)
            const int* const* walks = walk_pays(W.mode, c.max_rows(feats.rows), feats.cols, c.max_rows(nq)) ? level_walks(c, B, W, blk.layer + 1) : nullptr;
            for (int g = 0; g < c.G; ++g) {
                const pcrcg_table& t = B.b[g]->pools[blk.layer];
                jobs[g] = GatherJob{feats.p[g], t.idx, sc.p[g], feats.rows[g], nq[g], t.cols, t.ld, walks ? walks[g] : nullptr};
            }
            c.check(gather_max_multi(jobs, c.G, feats.cols, c.st));
        }
    }
    if (blk.shortcut) {
        Mat s2 = c.gemm_out(nq, blk.out_dim, sc.cols);
        Stat s2s = stat_buffer(c, nq, blk.out_dim);
        linear(c, sc, blk.shortcut, sc.cols, nullptr, s2, &s2s);
        norm_act(c, u2, 0.1f, y, &u2s, &s2, true, &s2s);      // lrelu(IN(unary2) + IN(shortcut))
    } else {
        norm_act(c, u2, 0.1f, y, &u2s, &sc, false);           // lrelu(IN(unary2) + shortcut)
    }
    c.release(m);
    return y;
}

// x_out = lrelu(IN2d(max_j e), 0.2) for e[i,j,:] = cn[i, :cw] + cn[idx[i,j], cw:2cw]: reduction + normalisation
// (max commutes with the monotone normalise + LeakyReLU); statistics as fp64 sums when the widths allow, else as pairs
void edge_norm(Ctx& c, const float* cn, int ld_cn, int cw, const int* idx, int n, int k, float* emax, int ld_emax, float* out,
               int ld_out, void* sums, bool sums_ok, float* stats, void* ws, size_t wsb) {
    if (sums && sums_ok) {
        c.check(pcrcg_edgeconv_reduce_sums(cn, ld_cn, cn + cw, ld_cn, idx, n, k, cw, emax, ld_emax, sums, c.st));
        c.check(pcrcg_instnorm_apply_sums(emax, n, cw, ld_emax, sums, (double)n * (double)k, 1e-5f, nullptr, 0, nullptr, 0.2f, out,
                                          ld_out, c.st));
        return;
    }
    c.check(pcrcg_edgeconv_reduce(cn, ld_cn, cn + cw, ld_cn, idx, n, k, cw, 1e-5f, emax, ld_emax, stats, ws, wsb, c.st));
    c.check(pcrcg_instnorm_apply(emax, n, cw, ld_emax, stats, nullptr, 0, nullptr, 0.2f, out, ld_out, c.st));
}

// edge_norm for every cloud of the call: the reductions of all of them in ONE launch where the row-parallel kernel applies
void edge_norm_all(Ctx& c, const Mat& cn, int cw, int* const* idx, const int* n, const int* k, const Mat& e, const Mat& out,
                   void* const* sums, bool sums_ok, float* stats, void* ws, size_t wsb) {
    bool multi = sums_ok;
    EdgeCloud cl[GMAX];
    for (int g = 0; g < c.G; ++g) {
        multi = multi && sums[g] != nullptr;
        cl[g] = EdgeCloud{cn.p[g], cn.p[g] + cw, idx[g], e.p[g], static_cast<double*>(sums[g]), n[g], k[g]};
    }
    if (multi && edgeconv_rows_ok(cl, c.G, cn.ld, cn.ld, e.ld, cw)) {
        c.check(edgeconv_rows_multi(cl, c.G, cn.ld, cn.ld, e.ld, cw, true, nullptr, c.st));
        NormJobs nj = norm_jobs(c, e, sums, out);       // (e has the clouds' n rows; the statistics are over n k edges)
        bool one = nj.aligned;
        for (int g = 0; g < c.G; ++g) {
            nj.j[g].count = (double)n[g] * (double)k[g];
            one = one && n[g] > 0 && k[g] > 0;
        }
        apply_sums(c, nj.j, one, cw, e.ld, 0, 0.2f, out.ld);
        return;
    }
    for (int g = 0; g < c.G; ++g)
        edge_norm(c, cn.p[g], cn.ld, cw, idx[g], n[g], k[g], e.p[g], e.ld, out.p[g], out.ld, sums[g], sums_ok, stats, ws, wsb);
}

// SelfAttention.forward (ref:models/gcn.py:110-134) on row-major [n, ch]: one cloud of every pair
// knn_given: the clouds' kNN tables when the caller has them already (they depend on the coordinates only, which no layer
// changes: the forward computes them once for all self-attention layers), or NULL
Mat self_attention(Ctx& c, const pcrcg_model& mdl, const pcrcg_gnn_layer& gl, const float* const* coords, const Mat& f,
                   int* const* knn_given = nullptr) {
    const int ch = f.cols;
    Mat y = c.mat(f.rows, ch);
    const size_t m = c.mark();
    int kq[GMAX];
    int* idx[GMAX];
    for (int g = 0; g < c.G; ++g) {
        const int n = f.rows[g];
        kq[g] = mdl.knn_k < n - 1 ? mdl.knn_k : n - 1;
        idx[g] = knn_given ? knn_given[g] : static_cast<int*>(c.raw(sizeof(int) * (size_t)n * (kq[g] > 0 ? kq[g] : 1)));
    }
    Mat cat = c.mat(f.rows, 4 * ch);
    const size_t wsb = pcrcg_edgeconv_ws_bytes(2 * ch);
    void* ws = c.raw(wsb);
    float* stats = static_cast<float*>(c.raw(sizeof(float) * 4 * ch));
    Mat cn1 = c.gemm_out(f.rows, 2 * ch, ch), e1 = c.mat(f.rows, ch), cn2 = c.gemm_out(f.rows, 4 * ch, ch), e2 = c.mat(f.rows, 2 * ch);
    Mat x3 = c.gemm_out(f.rows, ch, 4 * ch);
    Stat x3s = stat_buffer(c, f.rows, ch);
    // InstanceNorm2d statistics of the two edge convolutions as fp64 sums (zero arena) when that form applies
    void *sums1[GMAX], *sums2[GMAX];
    for (int g = 0; g < c.G; ++g) {
        sums1[g] = gemm_split_terms_on() ? c.zraw(2 * sizeof(double) * (size_t)ch) : nullptr;
        sums2[g] = gemm_split_terms_on() ? c.zraw(2 * sizeof(double) * (size_t)(2 * ch)) : nullptr;
    }
    Mat cat1 = cols(cat, ch, ch), cat2 = cols(cat, 2 * ch, 2 * ch);
    const bool ok1 = sums_apply_ok(e1, cat1, nullptr), ok2 = sums_apply_ok(e2, cat2, nullptr);
    if (c.live()) {
        if (!knn_given)
            for (int g = 0; g < c.G; ++g) c.check(pcrcg_knn(coords[g], f.rows[g], kq[g], idx[g], c.st));
        c.check(copy2d_multi(f.p, cat.p, f.rows, c.G, f.ld, cat.ld, ch, c.st));                // x0, every cloud
        // x1 = max_k lrelu(IN2d(conv1(cat(f_i, f_j - f_i))))  (:121-125)
        linear(c, f, gl.edge1, ch, nullptr, cn1);
        edge_norm_all(c, cn1, ch, idx, f.rows, kq, e1, cat1, sums1, ok1, stats, ws, wsb);
        // x2 from x1 with conv2 (:127-129)
        linear(c, cat1, gl.edge2, ch, nullptr, cn2);
        edge_norm_all(c, cn2, 2 * ch, idx, f.rows, kq, e2, cat2, sums2, ok2, stats, ws, wsb);
        // x3 = lrelu(IN(conv3(cat(x0,x1,x2))))  (:131-132)
        linear(c, cat, gl.conv3, 4 * ch, nullptr, x3, &x3s);
    }
    norm_act(c, x3, 0.2f, y, &x3s);
    c.release(m);
    return y;
}

// x + AttentionalPropagation(x, src)  (ref:models/gcn.py:151-185, 213-214)
// q_given: the query projection of x, computed by the caller (both directions of a layer in one launch), or NULL
Mat cross_attention(Ctx& c, const pcrcg_model& mdl, const pcrcg_gnn_layer& gl, const Mat& x, const Mat& src, const Mat* q_given = nullptr) {
    const int ch = x.cols, h = mdl.heads, d = ch / h;
    Mat y = c.mat(x.rows, ch);
    const size_t m = c.mark();
    // the key and value projections read the same rows: ONE product of width 2 ch when the caller packed the two weight
    // matrices (and biases) behind each other (pcrcg_amd/runner.py does), k and v are then column blocks of its output
    const bool kv_fused = gl.wv == gl.wk + (size_t)ch * ch && gl.bv == gl.bk + ch;
    Mat q = q_given ? *q_given : c.gemm_out(x.rows, ch, ch), kk, v, msg = c.mat(x.rows, ch);
    if (kv_fused) {
        Mat kv = c.gemm_out(src.rows, 2 * ch, ch);
        linear(c, src, gl.wk, ch, gl.bk, kv);
        kk = cols(kv, 0, ch);
        v = cols(kv, ch, ch);
        kk.zeroed = v.zeroed = false;
    } else {
        kk = c.gemm_out(src.rows, ch, ch);
        v = c.gemm_out(src.rows, ch, ch);
    }
    Mat sc = c.mat(x.rows, c.max_rows(src.rows));
    Mat cat = c.mat(x.rows, 2 * ch), h0 = c.gemm_out(x.rows, 2 * ch, 2 * ch), h1 = c.mat(x.rows, 2 * ch), delta = c.gemm_out(x.rows, ch, 2 * ch);
    if (!q_given) linear(c, x, gl.wq, ch, gl.bq, q);
    if (!kv_fused) {
        linear(c, src, gl.wk, ch, gl.bk, kk);
        linear(c, src, gl.wv, ch, gl.bv, v);
    }
    bool att_done = false;
    if (c.live()) {       // every pair's attention in ONE launch where the matrix-core kernel applies (round 5)
        AttnCloud cl[GMAX];
        for (int g = 0; g < c.G; ++g) cl[g] = AttnCloud{q.p[g], kk.p[g], v.p[g], msg.p[g], x.rows[g], src.rows[g]};
        if (attention_mfma_ok(cl, c.G, q.ld, kk.ld, v.ld, d)) {
            c.check(attention_mfma_multi(cl, c.G, q.ld, kk.ld, v.ld, msg.ld, h, d, 1.0f / sqrtf((float)d), c.st));
            att_done = true;
        }
    }
    if (c.live())
        for (int g = 0; g < c.G; ++g) {
            const int n = x.rows[g], ms = src.rows[g];
            if (att_done) {
            } else if (pcrcg_attention_supported(d) && (long)n * ms <= 1000000) {
                // all heads in one launch (heads are contiguous column blocks after the weight permutation); a latency win on
                // the few hundred coarse points of an indoor pair (49 vs 138 us of kernels + 11 launches less per call,
                // scripts/attention_bench.py) -- beyond ~1000 x 1000 the GEMM path below is faster (1900 x 1900: 228 vs 640 us)
                c.check(pcrcg_attention(q.p[g], q.ld, kk.p[g], kk.ld, v.p[g], v.ld, msg.p[g], msg.ld, n, ms, h, d,
                                        1.0f / sqrtf((float)d), c.st));
            } else {
                for (int i = 0; i < h; ++i) {
                    c.check(pcrcg_gemm_f32(q.p[g] + i * d, q.ld, kk.p[g] + i * d, kk.ld, 1, sc.p[g], ms, n, ms, d, nullptr, nullptr,
                                           c.st));
                    c.check(pcrcg_softmax_rows(sc.p[g], n, ms, ms, 1.0f / sqrtf((float)d), c.st));
                    c.check(pcrcg_gemm_f32(sc.p[g], ms, v.p[g] + i * d, v.ld, 0, msg.p[g] + i * d, msg.ld, n, d, ms, nullptr, nullptr,
                                           c.st));
                }
            }
        }
    if (c.live()) c.check(copy2d_multi(x.p, cat.p, x.rows, c.G, x.ld, cat.ld, ch, c.st));
    linear(c, msg, gl.wm, ch, gl.bm, cols(cat, ch, ch));       // merge, written next to x: cat([x, message])
    Stat h0s = stat_buffer(c, x.rows, 2 * ch);
    linear(c, cat, gl.w0, 2 * ch, gl.b0, h0, &h0s);
    if (!linear_norm(c, h0, &h0s, 0.0f, gl.w3, 2 * ch, gl.b3, delta)) {      // InstanceNorm1d + ReLU, inside w3's A loads
        norm_act(c, h0, 0.0f, h1, &h0s);
        linear(c, h1, gl.w3, 2 * ch, gl.b3, delta);
    }
    if (c.live())
        for (int g = 0; g < c.G; ++g) c.check(pcrcg_add(x.p[g], delta.p[g], y.p[g], (long)x.rows[g] * ch, c.st));
    c.release(m);
    return y;
}

void forward(Ctx& c, const pcrcg_model& mdl, const Batches& B, const pcrcg_outputs* out) {
    const int L = B.b[0]->n_levels;
    c.bf16 = mdl.feature_bf16 != 0;
    Mat x;
    for (int g = 0; g < c.G; ++g) {
        x.p[g] = const_cast<float*>(B.b[g]->features);
        x.rows[g] = B.b[g]->n_points[0];
    }
    x.cols = x.ld = B.b[0]->feat_dim;
    std::vector<Mat> skips;
    // the gathers' query walks: sum n_points ints per pair, taken before the blocks so that the arena stays a stack
    Walks W;
    W.mode = debug_opts().walk;
    if (W.mode)
        for (int l = 0; l < L; ++l)
            for (int g = 0; g < c.G; ++g) {
                const int n = B.b[g]->n_points[l];
                W.w[l][g] = static_cast<int*>(c.raw(sizeof(int) * (size_t)(n > 0 ? n : 1)));
            }
    // 1. encoder (:519-524)
    for (int i = 0; i < mdl.n_enc; ++i) {
        if (mdl.enc_skip[i]) skips.push_back(x);
        const pcrcg_block& blk = mdl.enc[i];
        x = blk.type == PCRCG_BLK_SIMPLE ? simple_block(c, B, W, blk, x) : resnet_block(c, B, W, blk, x);
    }
    // 2. bottleneck (:527-528) and 3. GNN (:532-536)
    const int gd = mdl.gnn_dim;
    int nc[GMAX] = {}, ns[GMAX] = {}, nt[GMAX] = {}, zero[GMAX] = {};
    const float *c0[GMAX], *c1[GMAX];
    for (int g = 0; g < c.G; ++g) {
        nc[g] = B.b[g]->n_points[L - 1];
        ns[g] = B.b[g]->len_src_c;
        nt[g] = nc[g] - ns[g];
        c0[g] = B.b[g]->points[L - 1];
        c1[g] = B.b[g]->points[L - 1] + 3 * (long)ns[g];
    }
    Mat fc = c.gemm_out(nc, gd, mdl.enc_out_dim);
    linear(c, x, mdl.bottle_w, mdl.enc_out_dim, mdl.bottle_b, fc);
    Mat d0 = rows(fc, zero, ns), d1 = rows(fc, ns, nt);
    // the kNN graphs of the coarse clouds: geometry only (ref:models/gcn.py:48-51 builds them from the coordinates in every
    // self-attention layer: the same tables each time) -- once per forward (round 5), order [source clouds | target clouds]
    int* knn0[GMAX] = {};
    int* knn1[GMAX] = {};
    int n_self = 0;
    for (int i = 0; i < mdl.n_gnn; ++i) n_self += mdl.gnn[i].cross ? 0 : 1;
    const bool knn_once = n_self >= 2;
    if (knn_once)
        for (int g = 0; g < c.G; ++g) {
            const int k0 = mdl.knn_k < ns[g] - 1 ? mdl.knn_k : ns[g] - 1, k1 = mdl.knn_k < nt[g] - 1 ? mdl.knn_k : nt[g] - 1;
            knn0[g] = static_cast<int*>(c.raw(sizeof(int) * (size_t)ns[g] * (k0 > 0 ? k0 : 1)));
            knn1[g] = static_cast<int*>(c.raw(sizeof(int) * (size_t)nt[g] * (k1 > 0 ? k1 : 1)));
            if (c.live()) {
                c.check(pcrcg_knn(c0[g], ns[g], k0, knn0[g], c.st));
                c.check(pcrcg_knn(c1[g], nt[g], k1, knn1[g], c.st));
            }
        }
    // Both clouds of every pair through one pass of 2 G clouds where a layer treats them alike, stacked() [source clouds |
    // target clouds].  The multi-cloud kernels take four clouds, so this applies to calls of one or two pairs; with more
    // pairs per call the two sides run as two passes.
    const int G0 = c.G;
    const bool stack = 2 * G0 <= GMAX && gemm_split_terms_on();
    const float* c01[GMAX] = {};
    int* knn01[GMAX] = {};
    for (int g = 0; g < G0 && stack; ++g) { c01[g] = c0[g]; c01[G0 + g] = c1[g]; knn01[g] = knn0[g]; knn01[G0 + g] = knn1[g]; }
    for (int i = 0; i < mdl.n_gnn; ++i) {
        const pcrcg_gnn_layer& gl = mdl.gnn[i];
        if (gl.cross) {
            // the second direction's queries come from d1, which the first direction does not change: both query
            // projections in one launch (2 G products sharing wq)
            Mat q0, q1;
            if (stack) {
                const int ch = d0.cols;
                const Mat x2 = stacked(d0, d1, G0);
                const Mat q2 = c.twice([&] { Mat q = c.gemm_out(x2.rows, ch, ch); linear(c, x2, gl.wq, ch, gl.bq, q); return q; });
                q0 = half(q2, 0, G0);
                q1 = half(q2, 1, G0);
            }
            // (the results are allocated above the projections: the arena is a stack, so they stay until the forward ends)
            d0 = cross_attention(c, mdl, gl, d0, d1, stack ? &q0 : nullptr);
            d1 = cross_attention(c, mdl, gl, d1, d0, stack ? &q1 : nullptr);   // sees the updated d0 (:214)
        } else if (stack) {
            // The layer is applied to the source cloud and to the target cloud of every pair with the SAME weights and no
            // exchange between them (ref:models/gcn.py:207-211): every weight product of the layer once for all 2 G clouds
            // (round 5: three launches per layer instead of six; the per-cloud kernels are unchanged).
            const Mat f2 = stacked(d0, d1, G0);
            const Mat y2 = c.twice([&] { return self_attention(c, mdl, gl, c01, f2, knn_once ? knn01 : nullptr); });
            d0 = half(y2, 0, G0);
            d1 = half(y2, 1, G0);
        } else {
            d0 = self_attention(c, mdl, gl, c0, d0, knn_once ? knn0 : nullptr);
            d1 = self_attention(c, mdl, gl, c1, d1, knn_once ? knn1 : nullptr);
        }
    }
    // coarse features [score | saliency | proj_gnn feats] (:538-565), rows 16-byte aligned
    const int wc = gd + 2;
    Mat xc = c.mat(nc, wc, pad4(wc));
    {
        const size_t m = c.mark();
        Mat gcat = c.mat(nc, gd), fn = c.mat(nc, gd);
        Mat pst = c.mat(ns, c.max_rows(nt)), pts = c.mat(nt, c.max_rows(ns));
        if (c.live())
            for (int g = 0; g < c.G; ++g) {
                c.check(pcrcg_copy2d(d0.p[g], d0.ld, gcat.p[g], gcat.ld, ns[g], gd, c.st));
                c.check(pcrcg_copy2d(d1.p[g], d1.ld, gcat.p[g] + (long)ns[g] * gcat.ld, gcat.ld, nt[g], gd, c.st));
            }
        Mat feats = cols(xc, 2, gd), score = cols(xc, 0, 1), sal = cols(xc, 1, 1);
        linear(c, gcat, mdl.proj_gnn_w, gd, mdl.proj_gnn_b, feats);           // :538
        linear(c, feats, mdl.proj_score_w, gd, mdl.proj_score_b, score);      // :539
        if (c.live())
            for (int g = 0; g < c.G; ++g) {
                c.check(pcrcg_l2norm_rows(feats.p[g], feats.ld, fn.p[g], fn.ld, nc[g], gd, c.st));   // :541
                const float inv_t = 1.0f / mdl.temperature;
                const float* fs = fn.p[g];
                const float* ft = fn.p[g] + (long)ns[g] * fn.ld;
                // s1 = softmax(inner/T) @ tgt_scores, s2 = softmax(inner^T/T) @ src_scores  (:562-563); the softmax and
                // the product with the score column are one pass over each inner-product matrix
                c.check(pcrcg_gemm_f32(fs, fn.ld, ft, fn.ld, 1, pst.p[g], nt[g], ns[g], nt[g], gd, nullptr, nullptr, c.st));
                c.check(pcrcg_softmax_matvec(pst.p[g], ns[g], nt[g], nt[g], inv_t, score.p[g] + (long)ns[g] * xc.ld, xc.ld, sal.p[g],
                                             xc.ld, c.st));
                c.check(pcrcg_gemm_f32(ft, fn.ld, fs, fn.ld, 1, pts.p[g], ns[g], nt[g], ns[g], gd, nullptr, nullptr, c.st));
                c.check(pcrcg_softmax_matvec(pts.p[g], nt[g], ns[g], ns[g], inv_t, score.p[g], xc.ld, sal.p[g] + (long)ns[g] * xc.ld,
                                             xc.ld, c.st));
            }
        c.release(m);
    }
    x = xc;
    // 4. decoder (:567-570)
    // `x` may be LAZY between two decoder stages: the raw output of a unary's products whose InstanceNorm + LeakyReLU the
    // next stage's gathering product applies on load (xs = its column sums); materialise() applies it for anyone else
    Stat xs;
    bool lazy = false;
    auto materialise = [&]() {
        if (!lazy) return;
        Mat y = c.mat(x.rows, x.cols);
        norm_act(c, x, 0.1f, y, &xs);
        x = y;
        lazy = false;
    };
    for (int j = 0; j < mdl.n_dec; ++j) {
        const pcrcg_block& blk = mdl.dec[j];
        if (blk.type == PCRCG_BLK_UPSAMPLE) {
            const pcrcg_table* tabs[GMAX];
            int trows[GMAX] = {};
            for (int g = 0; g < c.G; ++g) { tabs[g] = &B.b[g]->upsamples[blk.layer - 1]; trows[g] = tabs[g]->rows; }
            const bool concat = j + 1 < mdl.n_dec && mdl.dec_concat[j + 1];
            const int cs = concat ? skips.back().cols : 0;
            const pcrcg_block* next = j + 1 < mdl.n_dec ? &mdl.dec[j + 1] : nullptr;
            // nearest_upsample -> cat(skip) -> unary as TWO products into one output: the unary's first columns on rows
            // of x gathered through the table (closest_pool, the shadow index reads a zero row), plus its skip columns on
            // the skip features.  Neither the upsampled matrix nor the concatenation is written: at level 0 that is
            // 31 + 61 MB of stores and 92 MB of loads that the product no longer waits for.
            if (concat && next && next->mlp_skip && next->skip_dim == cs && gemm_split_terms_on() &&
                (next->type == PCRCG_BLK_UNARY || next->type == PCRCG_BLK_LAST_UNARY) && x.ld % 4 == 0 &&
                skips.back().ld % 4 == 0) {
                const Mat& sk = skips.back();
                const bool last = next->type == PCRCG_BLK_LAST_UNARY;
                Mat tt = c.mat(trows, next->out_dim, pad4(next->out_dim));    // rows 16-byte aligned: it may be read normalised next
                if (lazy && !(gemm_split_terms_on() && lazy_stats_ready(c, x, &xs))) materialise();
                // nearest_upsample commutes with the linear map: the unary's first columns are applied to the COARSE rows
                // (with the producer's normalisation on load when lazy) and the product's rows copied up through the table,
                // the shadow index giving a zero row (no bias: what a zero input row maps to) -- a fine row repeated its
                // coarse row's product before, 4-5 times the flops and a random row gather per fine row.  Then the skip
                // part on top.
                Mat z = c.gemm_out(x.rows, next->out_dim, x.cols, pad4(next->out_dim));
                Fold up, add;
                up.sums = lazy ? &xs : nullptr;
                up.slope = 0.1f;
                add.accumulate = true;
                linear(c, x, next->mlp, next->mlp_ld, nullptr, z, z.zeroed, nullptr, nullptr, &up);
                if (c.live()) {          // every pair's rows in one launch
                    FirstJob jobs[GMAX];
                    for (int g = 0; g < c.G; ++g) jobs[g] = FirstJob{z.p[g], tabs[g]->idx, tt.p[g], z.rows[g], trows[g], tabs[g]->ld};
                    c.check(gather_first_multi(jobs, c.G, z.cols, z.ld, tt.ld, c.st));
                }
                linear(c, sk, next->mlp_skip, next->mlp_skip_ld, nullptr, tt, /*c_zeroed=*/true, nullptr, nullptr, &add);
                skips.pop_back();
                lazy = false;
                x = tt;
                if (!last) {                                         // its normalisation is left to the next consumer
                    xs = stat_buffer(c, tt.rows, tt.cols);           // (filled by one pass over tt: two products wrote it)
                    lazy = true;
                }
                ++j;                                                 // the unary block is done
                continue;
            }
            materialise();
            Mat y = c.mat(trows, x.cols + cs, pad4(x.cols + cs));
            Mat xd = x;
            if (x.ld != x.cols) {   // gather_first reads dense rows
                xd = c.mat(x.rows, x.cols);
                if (c.live())
                    for (int g = 0; g < c.G; ++g) c.check(pcrcg_copy2d(x.p[g], x.ld, xd.p[g], xd.ld, x.rows[g], x.cols, c.st));
            }
            if (c.live())
                for (int g = 0; g < c.G; ++g) {
                    c.check(pcrcg_gather_first(xd.p[g], xd.rows[g], xd.cols, tabs[g]->idx, tabs[g]->rows, tabs[g]->ld, y.p[g], y.ld, c.st));
                    if (concat) {
                        const Mat& s = skips.back();
                        c.check(pcrcg_copy2d(s.p[g], s.ld, y.p[g] + x.cols, y.ld, s.rows[g], s.cols, c.st));
                    }
                }
            if (concat) skips.pop_back();
            x = y;
        } else if (blk.type == PCRCG_BLK_UNARY) {
            materialise();
            Mat t = c.gemm_out(x.rows, blk.out_dim, x.cols), y = c.mat(x.rows, blk.out_dim);
            Stat ts = stat_buffer(c, t.rows, t.cols);
            linear(c, x, blk.mlp, blk.mlp_ld, nullptr, t, &ts);
            norm_act(c, t, 0.1f, y, &ts);
            x = y;
        } else {   // last_unary
            materialise();
            Mat y = c.mat(x.rows, blk.out_dim, pad4(blk.out_dim));
            linear(c, x, blk.mlp, blk.mlp_ld, nullptr, y);
            x = y;
        }
    }
    materialise();
    // heads (:571-582)
    if (c.live()) {
        const int fd = mdl.final_dim;
        float *ff[GMAX], *so[GMAX], *ss[GMAX];           // the three heads of every pair in one launch
        for (int g = 0; g < c.G; ++g) { ff[g] = out[g].feats_f; so[g] = out[g].scores_overlap; ss[g] = out[g].scores_saliency; }
        c.check(heads_multi(x.p, x.rows, c.G, x.ld, fd, ff, so, ss, c.st));
    }
}

int validate(const pcrcg_model* m, const pcrcg_batch* b) {
    PCRCG_CHECK_ARG(m && b);
    PCRCG_CHECK_ARG(m->n_enc >= 1 && m->n_enc <= PCRCG_MAX_BLOCKS && m->n_dec >= 1 && m->n_dec <= PCRCG_MAX_BLOCKS);
    PCRCG_CHECK_ARG(m->n_gnn >= 0 && m->n_gnn <= PCRCG_MAX_GNN);
    PCRCG_CHECK_ARG(b->n_levels >= 1 && b->n_levels <= PCRCG_MAX_LEVELS);
    PCRCG_CHECK_ARG(b->len_src_c >= 1 && b->len_src_c < b->n_points[b->n_levels - 1]);
    PCRCG_CHECK_ARG(m->heads >= 1 && m->gnn_dim % m->heads == 0 && m->temperature > 0.0f);
    for (int i = 0; i < m->n_enc; ++i) PCRCG_CHECK_ARG(m->enc[i].layer >= 0 && m->enc[i].layer + m->enc[i].strided < b->n_levels);
    // the first KPConv reads the features with their own width: the block's in_dim, or the cin_pad its kp_w_pad holds
    const pcrcg_block& b0 = m->enc[0];
    if (b->feat_dim != b0.in_dim && !(b0.kp_w_pad && b0.cin_pad > 0 && b->feat_dim == b0.cin_pad)) {
        set_error("pcrcg_kpfcnn_forward: bad argument: batch feat_dim %d is neither the first block's in_dim %d nor its cin_pad %d "
                  "(with kp_w_pad)", b->feat_dim, b0.in_dim, b0.kp_w_pad ? b0.cin_pad : 0);
        return PCRCG_EBADARG;
    }
    return PCRCG_OK;
}

int validate_group(const pcrcg_model* m, const pcrcg_batch* b, int n) {
    PCRCG_CHECK_ARG(b && n >= 1 && n <= GMAX);
    for (int g = 0; g < n; ++g) {
        PCRCG_PROPAGATE(validate(m, b + g));
        PCRCG_CHECK_ARG(b[g].n_levels == b[0].n_levels && b[g].feat_dim == b[0].feat_dim);
    }
    return PCRCG_OK;
}

}  // namespace
}  // namespace pcrcg

using namespace pcrcg;

extern "C" {

size_t pcrcg_kpfcnn_group_ws_bytes(const pcrcg_model* model, const pcrcg_batch* batches, int n) {
    if (validate_group(model, batches, n) != PCRCG_OK) return 0;
    Ctx c;
    c.dry = true;
    c.G = n;
    Batches B;
    for (int g = 0; g < GMAX; ++g) B.b[g] = g < n ? batches + g : nullptr;
    forward(c, *model, B, nullptr);
    return c.peak + c.zoff + 4096;
}

size_t pcrcg_kpfcnn_ws_bytes(const pcrcg_model* model, const pcrcg_batch* batch) {
    return pcrcg_kpfcnn_group_ws_bytes(model, batch, 1);
}

int pcrcg_kpfcnn_forward_group(const pcrcg_model* model, const pcrcg_batch* batches, const pcrcg_outputs* outs, int n, void* ws,
                               size_t ws_bytes, void* stream) {
    PCRCG_PROPAGATE(validate_group(model, batches, n));
    PCRCG_CHECK_ARG(outs && ws);
    for (int g = 0; g < n; ++g) PCRCG_CHECK_ARG(outs[g].feats_f && outs[g].scores_overlap && outs[g].scores_saliency);
    Batches B;
    for (int g = 0; g < GMAX; ++g) B.b[g] = g < n ? batches + g : nullptr;
    // pass 1 (no launches): how much of the workspace the zero arena takes for these batches
    Ctx d;
    d.dry = true;
    d.G = n;
    forward(d, *model, B, nullptr);
    if (d.zoff + d.peak > ws_bytes) {
        set_error("pcrcg_kpfcnn_forward: workspace too small (%zu needed, %zu given)", d.zoff + d.peak, ws_bytes);
        return PCRCG_EWORKSPACE;
    }
    Ctx c;
    c.G = n;
    c.zbase = static_cast<char*>(ws);
    c.zcap = d.zoff;
    c.base = c.zbase + d.zoff;
    c.cap = ws_bytes - d.zoff;
    c.st = as_stream(stream);
    if (d.zoff > 0) PCRCG_CHECK_HIP(hipMemsetAsync(ws, 0, d.zoff, c.st));
    forward(c, *model, B, outs);
    return c.rc;
}

int pcrcg_kpfcnn_forward(const pcrcg_model* model, const pcrcg_batch* batch, const pcrcg_outputs* out, void* ws,
                         size_t ws_bytes, void* stream) {
    return pcrcg_kpfcnn_forward_group(model, batch, out, 1, ws, ws_bytes, stream);
}
}
