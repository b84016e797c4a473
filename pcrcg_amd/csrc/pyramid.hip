// pyramid.hip -- host-side pyramid builder: the whole front end of one fragment pair or of several stacked into one chain
// (3 grid subsamplings, 4 cell grids, 10 radius searches, the tie-order restore step) enqueued by ONE C-ABI call from
// plain C arguments.  The counterpart of collate_fn_descriptor's pyramid loop (ref:datasets/dataloader.py:230-361) and of
// batch_grid_subsampling_kpconv / batch_neighbors_kpconv (:14-69); same sequence as pcrcg_amd/pyramid.py's
// pyramid_steps (the Python mirror, kept for calibration and for tie_order="reference"), which this replaces on the
// pipeline's hot path: ~85 launches cost one FFI crossing and ~0.3 ms of host time instead of ~1.7 ms of Python.
//
// No device code of its own but the probe kernels of pcrcg_stream_pipe_classes: it sequences grid_subsample_bound,
// pcrcg_cellgrid_build, radius_search, kdforest_build_levels (frontend.h) and pcrcg_radius_reorder_jobs over a
// caller-provided arena, in two steps around ONE host round trip.  pyramid_enqueue carves the arena and enqueues the chain:
// levels are sized from a row BOUND (pcrcg_pyramid_cfg::shrink), so nothing is read back between them, and every search is
// the cell-cooperative kernel alone (RadiusPass::first).  Then the tables' metadata and every level's cloud lengths come
// back through the caller's pinned scratch (MetaView); the call waits for an event of its own.  pyramid_finish launches the
// per-query redo kernel for the tables that ask for it (normally none; then the metadata is fetched once more), fills the
// pcrcg_batch structs and assembles the restore step, which it runs or hands to the caller (pcrcg_pyramid_restore).
// Builders on several host threads may share a stream: a call holds the stream's enqueue lock (g_enqueue, the only global
// state here) while it enqueues and lets go of it before it waits (pcrcg_amd/pairstream.py).
//
// Arena layout: persistent results first (points of all levels contiguous -- which is also the KD-forest's input,
// so nothing is concatenated later --, lengths [levels][nb], features, tables, per-table counts / tie rows, cell
// grids), then the subsamplings' scratch.  The input clouds are always copied into it (level 0's points too), so
// everything the returned pcrcg_batch points to lives in the arena.
#include <time.h>

#include <cmath>
#include <cstdlib>
#include <vector>

#include "frontend.h"

namespace pcrcg {
namespace {

inline double now_us() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e6 + ts.tv_nsec * 1e-3;
}

// ---- which streams share a hardware dispatcher (pcrcg_stream_pipe_classes) ----
// The command processor of gfx950 runs FOUR compute dispatchers ("pipes"); every HIP stream lives on a hardware queue of
// one of them, and a dispatcher hands out the workgroups of ONE kernel at a time: while a kernel of many workgroups is
// being dispatched -- for a GEMM beside other work that is most of its run time -- every other stream on the same dispatcher
// stands still (profiles/r06_queue_pipes.txt: a one-workgroup kernel completes in 12 us beside such a dispatch on another
// dispatcher and in ~470 us behind it on the same one; streams i and i + 4 share one, whatever GPU_MAX_HW_QUEUES says).
// That is the pair engine's "concurrency wall" of rounds 3-5: a fifth busy stream does not add concurrency, it halves two.
__global__ void k_probe_many(int* sink, int spin) {
    int x = threadIdx.x;
    for (int i = 0; i < spin; ++i) x = x * 1664525 + 1013904223;
    if (x == 0x7fffffff) sink[0] = x;
}
__global__ void k_probe_tiny(int* sink) {
    if (threadIdx.x == 1234567) sink[1] = 1;
}

// words src[0..n) (+ src2[0..n2)) -> h_scratch[1..]: async copies and an event on the stream, so the call waits for its
// own work only and several host threads can share one stream.  Returns when the words are there.  (`enqueue`: the
// stream's enqueue lock held by the caller, released once the transfer is in the stream, before the wait.)
int fetch(int* h_scratch, const int* src, int n, const int* src2, int n2, hipStream_t st,
          std::unique_lock<std::mutex>* enqueue = nullptr) {
    PCRCG_CHECK_HIP(hipMemcpyAsync(h_scratch + 1, src, sizeof(int) * n, hipMemcpyDeviceToHost, st));
    if (n2 > 0) PCRCG_CHECK_HIP(hipMemcpyAsync(h_scratch + 1 + n, src2, sizeof(int) * n2, hipMemcpyDeviceToHost, st));
    hipEvent_t ev;
    PCRCG_CHECK_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e = hipEventRecord(ev, st);
    if (enqueue && enqueue->owns_lock()) enqueue->unlock();
    if (e == hipSuccess) e = hipEventSynchronize(ev);
    (void)hipEventDestroy(ev);
    PCRCG_CHECK_HIP(e);
    return PCRCG_OK;
}

struct Arena {
    char* base;
    size_t cap, off = 0, peak = 0;
    bool dry;
    Arena(void* p, size_t bytes, bool dry_) : base(static_cast<char*>(p)), cap(bytes), dry(dry_) {}
    void* raw(size_t bytes) {
        bytes = (bytes + 255) & ~size_t(255);
        void* p = base ? base + off : nullptr;
        off += bytes;
        if (off > peak) peak = off;
        return p;
    }
    template <typename T>
    T* take(size_t count) { return static_cast<T*>(raw((count ? count : 1) * sizeof(T))); }
    bool ok() const { return dry || off <= cap; }
};

// One table of the pyramid: its search (the first pass and the redo pass launch the SAME descriptor; s.cols is the limit
// and the table's leading dimension, s.count / s.tie_rows feed the restore step) and where it goes in the batch.
struct TableRec {
    RadiusSearch s;
    int kind;                          // 0 conv (neighbors), 1 pool, 2 upsample
    int level, q_level, sup_level;     // level of the table in the batch; levels whose points are the queries / the supports
};

// The metadata words of one build, in the order pyramid_enqueue lays them out on the device and ONE fetch brings them to
// the host: for each of the 3 L table slots [max_count of each of the P output batches, status, tie_rows], then the
// L subsampled row counts, then the "a level outgrew its bound" word -- and, from their own place on the device, the
// [L][nb] cloud lengths behind them.  Over the device block only addresses are taken, over the host copy values are read.
struct MetaView {
    int* w; int P, L;
    struct Table {
        int* w; int P;
        int& max_count(int p) const { return w[p]; }
        int& status() const { return w[P]; }
        int& tie_rows() const { return w[P + 1]; }
        int widest() const { int m = 0; for (int p = 0; p < P; ++p) m = w[p] > m ? w[p] : m; return m; }
    };
    Table table(int i) const { return Table{w + (P + 2) * i, P}; }
    int* row_counts() const { return w + (P + 2) * 3 * L; }
    int& overflow() const { return row_counts()[L]; }
    int words() const { return (P + 2) * 3 * L + L + 1; }      // (without the lengths)
    const int* lengths() const { return w + words(); }
};
}  // namespace
}  // namespace pcrcg

using namespace pcrcg;

// events of one call (stream fork / join); destroyed when the call returns -- a recorded wait keeps what it needs
struct EventBox {
    std::vector<hipEvent_t> ev;
    int make(hipEvent_t* e) {
        PCRCG_CHECK_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
        ev.push_back(*e);
        return PCRCG_OK;
    }
    ~EventBox() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
};

// The input clouds may come in several PARTS (the pairs of a grouped build, each where its caller left it): part i holds
// n_parts[i] rows and nb_parts[i] cloud lengths; they are copied behind each other into the arena (the builder copies its
// input anyway), so stacking pairs costs no concatenation kernel on the caller's side.
struct Parts {
    const float* const* pts;
    const int* n;
    const int* const* len;
    const int* nb;
    int count;
};

// Row bound of every level: level 0 holds n0 rows, a subsampled level at most `shrink` times the bound of the level it
// comes from (the caller's promise, pcrcg_pyramid_cfg::shrink; a cloud that keeps more is reported as PCRCG_EWORKSPACE).
// Everything on the device is SIZED by these bounds -- buffers, tables, launch grids -- and every kernel reads the
// actual row counts from the cloud lengths, which never leave the device until the end of the chain.
static void level_caps(int n0, const pcrcg_pyramid_cfg* cfg, int* cap) {
    double shrink = cfg->shrink;
    if (!(shrink > 0.0) || shrink > 1.0) shrink = 1.0;
    cap[0] = n0;
    for (int l = 1; l < cfg->n_levels; ++l) {
        const double c = ceil((double)cap[l - 1] * shrink);
        cap[l] = c < 1.0 ? 1 : (c > (double)cap[l - 1] ? cap[l - 1] : (int)c);
    }
}

// The enqueue lock of a stream: held while a call enqueues its chain, released before it waits for its round trip, so the
// chains of several host threads stay whole in the stream while one call's wait overlaps the next call's enqueue.
struct EnqueueLocks {
    std::mutex mu;
    hipStream_t key[16];
    std::mutex lock[16];
    int n = 0;
    std::mutex* of(hipStream_t st) {
        std::lock_guard<std::mutex> g(mu);
        for (int i = 0; i < n; ++i)
            if (key[i] == st) return &lock[i];
        if (n == 16) return &lock[15];
        key[n] = st;
        return &lock[n++];
    }
};
static EnqueueLocks g_enqueue;

// ints the call uses of the caller's h_scratch: a reserved word (h_scratch[0], not written), MetaView's words and the L nb
// cloud lengths (P = output batches).  The argument checks of pyramid_build_checked (L <= 4 from 3 L <= PCRCG_MAX_REORDER_JOBS, P + 2 <= 16, L nb <= 64) bound it
// by 254 (L = 4, nb = 14, group = 1): within the 256 ints include/pcrcg.h asks for.
constexpr int kHostScratchInts = 256;
static int host_scratch_ints(int nb, const pcrcg_pyramid_cfg* cfg) {
    const int L = cfg->n_levels, P = cfg->group > 0 ? nb / cfg->group : 1;
    return 1 + MetaView{nullptr, P, L}.words() + L * nb;
}


// What pyramid_enqueue leaves for pyramid_finish: where things are in the arena, and what is in the streams.
struct Build {
    int nb, group;                                     // clouds, clouds per output batch (0: all in one)
    bool want_ties, one_forest;
    int cap[PCRCG_MAX_LEVELS];                         // row bound of every level (level_caps)
    float* level_pts[PCRCG_MAX_LEVELS];
    int* lens_all;                                     // [L][nb] cloud lengths
    float* feats;
    MetaView meta;                                     // the device block
    int* tie_status;                                   // the restore step's status word, behind it
    std::vector<TableRec> tables;
    void* forest[2] = {nullptr, nullptr};              // [0] level 0 (one_forest: all levels), [1] levels 1 .. L-1
    int forest_ns[2] = {0, 0}, forest_nb[2] = {0, 0};
    EventBox events;
    hipEvent_t forests_done = nullptr;                 // recorded behind the forests where they have a stream of their own
};

// Step 1: carve the arena and enqueue the whole chain.  A.dry: carve only (pcrcg_pyramid_ws_bytes; `in` is not read).
static int pyramid_enqueue(const Parts& in, int n0, int nb, const pcrcg_pyramid_cfg* cfg, Arena& A, hipStream_t st, Build& B) {
    const int L = cfg->n_levels;
    const bool dry = A.dry, want_ties = B.want_ties = cfg->tie_order != 0;
    const int group = B.group = cfg->group > 0 ? cfg->group : 0;
    B.nb = nb;
    int* const cap = B.cap;
    float** const level_pts = B.level_pts;
    level_caps(n0, cfg, cap);
    // ---- persistent block 1: points of all levels (level l at its own bound-sized place), lengths, features, metadata ----
    // (one block, every level a whole number of ROWS behind the first: the upper levels' forest indexes them as one array)
    {
        size_t rows = 0;
        for (int l = 0; l < L; ++l) rows += (size_t)cap[l] + 1;
        float* pts_all = A.take<float>(3 * rows);
        rows = 0;
        for (int l = 0; l < L; ++l) { level_pts[l] = pts_all + 3 * rows; rows += (size_t)cap[l] + 1; }
    }
    int* const lens_all = B.lens_all = A.take<int>((size_t)L * nb);
    float* const feats = B.feats = A.take<float>((size_t)n0);
    MetaView& meta = B.meta = MetaView{nullptr, group > 0 ? nb / group : 1, L};
    const size_t meta_ints = (size_t)meta.words() + 1;                // + the restore step's status word
    meta.w = A.take<int>(meta_ints);
    B.tie_status = &meta.overflow() + 1;
    if (!A.ok()) return PCRCG_EWORKSPACE;

    std::vector<TableRec>& tables = B.tables;
    tables.reserve(3 * L);
    if (!dry) {
        PCRCG_CHECK_HIP(hipMemsetAsync(meta.w, 0, sizeof(int) * meta_ints, st));
        size_t row = 0, cloud = 0;
        for (int i = 0; i < in.count; ++i) {
            if (in.n[i] > 0)
                PCRCG_CHECK_HIP(hipMemcpyAsync(level_pts[0] + 3 * row, in.pts[i], sizeof(float) * 3 * (size_t)in.n[i], hipMemcpyDeviceToDevice, st));
            PCRCG_CHECK_HIP(hipMemcpyAsync(lens_all + cloud, in.len[i], sizeof(int) * in.nb[i], hipMemcpyDeviceToDevice, st));
            row += (size_t)in.n[i];
            cloud += (size_t)in.nb[i];
        }
        PCRCG_CHECK_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(feats), 0x3f800000, (size_t)(n0 > 0 ? n0 : 1), st));
    }

    // ---- streams.  The chain is a DAG, not a line: a level's SUBSAMPLING needs only the level's points; the level's cell
    // grid and its conv search need them too and nothing from the subsampling; only the pool / upsample searches and the
    // next level need both.  And a KD-forest (restore step) needs only its levels' points.  With side streams from the
    // caller (pcrcg_pyramid_cfg::side_stream / side_stream2) the three subsamplings run back to back on the first from the
    // moment the input is in place -- beside grid 0 and the conv search of level 0, the longest kernel of the chain -- and
    // the forests on the second (or behind the subsamplings on the first); `st` keeps the grids and the ten searches and
    // waits, level by level, for the subsampled points.  Without side streams everything is enqueued on `st` in an order
    // that is valid for one stream (what rounds 2-5 did).
    // Two forests: level 0's, built as soon as the input is in place, and one over the subsampled levels, built when the
    // last of them exists.  Level 0 holds three quarters of the rows and the deepest trees.  (One forest PER level, one
    // launch each, was measured first: four persistent launches one after the other cost 3.9 ms of forest time per
    // four-pair chain against 1.1 for one launch -- the levels' critical paths add up instead of overlapping.)
    // Tie rows are the rule (every two-point cell of a subsampling puts one into the pool table), so the builds do not
    // wait to be told that there are some.
    hipStream_t sub_st = cfg->side_stream ? as_stream(cfg->side_stream) : st;
    hipStream_t f_st = cfg->side_stream2 ? as_stream(cfg->side_stream2) : sub_st;
    // b waits for everything enqueued on a so far
    auto order = [&](hipStream_t a, hipStream_t b) -> int {
        if (a == b || dry) return PCRCG_OK;
        hipEvent_t ev;
        PCRCG_PROPAGATE(B.events.make(&ev));
        PCRCG_CHECK_HIP(hipEventRecord(ev, a));
        PCRCG_CHECK_HIP(hipStreamWaitEvent(b, ev, 0));
        return PCRCG_OK;
    };
    // In line (no stream of their own) ONE forest over all levels, built when the last level exists: the levels' trees then
    // grow side by side in one persistent launch (1.07 ms per four-pair chain in the engine against 2 x 0.6 for two launches).
    const bool one_forest = B.one_forest = !want_ties || f_st == st || L < 2;
    int level_base[PCRCG_MAX_LEVELS] = {};               // row of level l relative to the first level of its forest
    auto build_forest = [&](int which) -> int {        // 0: level 0, 1: levels 1 .. L-1, 2: all levels (-> forest[0])
        if (!want_ties || (which == 1 && L < 2)) return PCRCG_OK;
        const int first = which == 1 ? 1 : 0, last = which == 0 ? 0 : L - 1, slot = which == 1 ? 1 : 0;
        for (int l = first; l <= last; ++l) level_base[l - first] = (int)((level_pts[l] - level_pts[first]) / 3);
        B.forest_ns[slot] = level_base[last - first] + cap[last];
        B.forest_nb[slot] = (last - first + 1) * nb;
        const size_t bytes = pcrcg_kdforest_ws_bytes(B.forest_ns[slot], B.forest_nb[slot]);
        B.forest[slot] = A.raw(bytes);
        if (!A.ok()) return PCRCG_EWORKSPACE;
        if (dry) return PCRCG_OK;
        PCRCG_PROPAGATE(order(which == 0 ? st : sub_st, f_st));       // the input copies / the last subsampling
        return kdforest_build_levels(level_pts[first], B.forest_ns[slot], lens_all + (size_t)first * nb, B.forest_nb[slot],
                                     last > first ? nb : 0, level_base, B.forest[slot], bytes, f_st);
    };

    // nq / ns are the BOUNDS of the query / support level (grids and tables are carved for them)
    auto add_table = [&](int kind, int level, int q_level, const void* grid, const void* qgrid, float radius, const float* q,
                         const int* qlen, int nq, int ns, const int* slen, int limit, int sup_level) -> int {
        const MetaView::Table m = meta.table((int)tables.size());
        TableRec t;
        t.kind = kind; t.level = level; t.q_level = q_level; t.sup_level = sup_level;
        RadiusSearch& s = t.s;
        s.q = q; s.nq = nq; s.qlen = qlen; s.qgrid = qgrid; s.sgrid = grid; s.ns = ns; s.slen = slen;
        s.nb = nb; s.group = group; s.radius = radius; s.cols = limit;
        s.idx = A.take<int64_t>((size_t)nq * limit);
        s.count = want_ties ? A.take<int>((size_t)nq) : nullptr;     // untruncated list lengths (tie restore cross-check)
        s.tie_rows = want_ties ? A.take<int>((size_t)nq) : nullptr;  // rows holding a tie
        s.max_count = &m.max_count(0); s.status = &m.status(); s.tie_count = want_ties ? &m.tie_rows() : nullptr;
        if (!A.ok()) return PCRCG_EWORKSPACE;
        // first pass only (the cell-cooperative search): rows with more than 128 hits (kCellListCap) and rows of a cell whose
        // neighbourhood does not fit LDS are marked and announced in the metadata; whether any table has one is known
        // with the metadata round trip, and only then (normally never) pyramid_finish launches the redo pass
        if (!dry) PCRCG_PROPAGATE(radius_search(s, RadiusPass::first, st));
        tables.push_back(t);
        return PCRCG_OK;
    };
    auto build_grid = [&](const float* sup, int ns, const int* slen, float radius, void** grid) -> int {
        const size_t gb = pcrcg_cellgrid_ws_bytes(ns, nb);
        *grid = A.raw(gb);
        if (!A.ok()) return PCRCG_EWORKSPACE;
        if (!dry) PCRCG_PROPAGATE(pcrcg_cellgrid_build(sup, ns, slen, nb, radius, *grid, gb, st));
        return PCRCG_OK;
    };

    // the subsamplings' scratch: ONE block for all levels (they run one after the other on one stream; level 0 needs the
    // most).  It is NOT handed back to the arena: beside the searches on another stream nothing may share its memory.
    const size_t sub_wsb = L > 1 ? pcrcg_grid_subsample_ws_bytes(cap[0], nb) : 0;
    void* sub_ws = L > 1 ? A.raw(sub_wsb) : nullptr;
    if (!A.ok()) return PCRCG_EWORKSPACE;

    void* carried = nullptr;
    float carried_r = 0.f;
    PCRCG_PROPAGATE(order(st, sub_st));                  // the input is in place: the subsamplings may start
    if (!one_forest || L == 1) PCRCG_PROPAGATE(build_forest(0));
    for (int l = 0; l < L; ++l) {
        const int limit = cfg->limit[l];
        const float r_conv = cfg->r_conv[l], r_pool = cfg->r_pool[l];
        float* pts = level_pts[l];
        int* lens = lens_all + (size_t)l * nb;
        const int n = cap[l];
        void* grid = nullptr;
        float grid_r = 0.f;
        const bool pooled = cfg->pooled[l] && l + 1 < L;
        if (!pooled && l + 1 < L) {
            set_error("pcrcg_pyramid_build: level %d of %d is not pooled", l, L);
            return PCRCG_EBADARG;
        }
        // the level's subsampling first: on its own stream it runs beside the grid and the conv search below
        if (pooled && !dry)
            PCRCG_PROPAGATE(grid_subsample_bound(pts, n, lens, nb, cfg->dl[l], 0, level_pts[l + 1], lens + nb, meta.row_counts() + l,
                                                 cap[l + 1], &meta.overflow(), sub_ws, sub_wsb, sub_st));
        if (pooled && l + 2 == L) PCRCG_PROPAGATE(build_forest(one_forest ? 2 : 1));      // the last subsampled level exists
        if (cfg->has_conv[l]) {
            if (carried && carried_r == r_conv) { grid = carried; grid_r = carried_r; }
            else { PCRCG_PROPAGATE(build_grid(pts, n, lens, r_conv, &grid)); grid_r = r_conv; }
            PCRCG_PROPAGATE(add_table(0, l, l, grid, grid, r_conv, pts, lens, n, n, lens, limit, l));
        }
        carried = nullptr;
        if (pooled) {
            float* sub = level_pts[l + 1];
            int* sub_len = lens + nb;
            const int m = cap[l + 1];
            if (grid == nullptr || grid_r != r_pool) {
                PCRCG_PROPAGATE(build_grid(pts, n, lens, r_pool, &grid));
                grid_r = r_pool;
            }
            PCRCG_PROPAGATE(order(sub_st, st));          // from here on `st` reads the subsampled level
            // the coarse level's grid first: it is the upsample table's support grid, the next level's conv grid AND the
            // query grid of the pool table (every query set of the pyramid walks a grid of its own, cell by cell)
            void* up_grid = nullptr;
            PCRCG_PROPAGATE(build_grid(sub, m, sub_len, 2 * r_pool, &up_grid));
            PCRCG_PROPAGATE(add_table(1, l, l + 1, grid, up_grid, r_pool, sub, sub_len, m, n, lens, limit, l));
            PCRCG_PROPAGATE(add_table(2, l, l, up_grid, grid, 2 * r_pool, pts, lens, n, m, sub_len, cfg->up_nearest ? 1 : limit, l + 1));
            carried = up_grid;
            carried_r = 2 * r_pool;
        }
    }
    if (!dry && want_ties && f_st != st) {
        PCRCG_PROPAGATE(B.events.make(&B.forests_done));
        PCRCG_CHECK_HIP(hipEventRecord(B.forests_done, f_st));
    }
    return PCRCG_OK;
}

// Step 2, after the ONE round trip of the call has brought MetaView's words and the cloud lengths to h_scratch + 1.
static int pyramid_finish(const Build& B, const pcrcg_pyramid_cfg* cfg, int* h_scratch, pcrcg_batch* out, int* h_lengths,
                          int* h_status, pcrcg_pyramid_restore* deferred, hipStream_t st) {
    const int L = B.meta.L, P = B.meta.P, nb = B.nb, group = B.group, nt = (int)B.tables.size();
    // whatever follows on `st` (the reorder step, the caller's readers, a second attempt in the same arena) comes after the forests
    if (B.forests_done) PCRCG_CHECK_HIP(hipStreamWaitEvent(st, B.forests_done, 0));
    const MetaView hm{h_scratch + 1, P, L};
    if (hm.overflow() != 0) {
        set_error("pcrcg_pyramid_build: a level keeps more rows than pcrcg_pyramid_cfg::shrink = %.3f allows -- call again with a "
                  "larger bound (1.0 always fits)", cfg->shrink);
        return PCRCG_EWORKSPACE;
    }
    for (int i = 0; i < L * nb; ++i) h_lengths[i] = hm.lengths()[i];
    int level_n[PCRCG_MAX_LEVELS];
    for (int l = 0; l < L; ++l) {
        level_n[l] = 0;
        for (int c = 0; c < nb; ++c) level_n[l] += h_lengths[(size_t)l * nb + c];
    }
    {   // tables with a row of more hits than the first pass stages (128 in the cell search, 256 in the per-query kernel): redo pass now, then the metadata once more (it appends tie rows)
        int redone = 0;
        for (int i = 0; i < nt; ++i) {
            const bool handed_over = (hm.table(i).status() & kRadiusRedoStatus) != 0;     // (the redo pass clears the bit)
            if (hm.table(i).widest() <= radius_fast_cap() && !handed_over) continue;
            PCRCG_PROPAGATE(radius_search(B.tables[i].s, RadiusPass::redo, st));
            ++redone;
        }
        if (redone) PCRCG_PROPAGATE(fetch(h_scratch, B.meta.w, hm.words(), B.lens_all, L * nb, st));
    }
    // rows of group p at level l: [row0, row0 + rows)
    auto group_rows = [&](int l, int p, int* row0, int* rows) {
        const int c0 = group > 0 ? p * group : 0, c1 = group > 0 ? c0 + group : nb;
        int a = 0, r = 0;
        for (int c = 0; c < c1; ++c) (c < c0 ? a : r) += h_lengths[(size_t)l * nb + c];
        *row0 = a;
        *rows = r;
    };
    for (int p = 0; p < P; ++p) {
        pcrcg_batch& o = out[p];
        o.n_levels = L;
        int row0, rows;
        group_rows(0, p, &row0, &rows);
        o.features = B.feats + row0;
        o.feat_dim = 1;
        o.len_src_c = h_lengths[(size_t)(L - 1) * nb + (group > 0 ? p * group : 0)];
        for (int l = 0; l < L; ++l) {
            group_rows(l, p, &row0, &rows);
            o.points[l] = B.level_pts[l] + 3 * (size_t)row0;
            o.n_points[l] = rows;
            o.stack_lengths[l] = B.lens_all + (size_t)l * nb + (group > 0 ? p * group : 0);
            o.neighbors[l] = pcrcg_table{nullptr, rows, 0, 1};
            o.pools[l] = pcrcg_table{nullptr, 0, 0, 1};
            o.upsamples[l] = pcrcg_table{nullptr, 0, 0, 1};
        }
    }
    pcrcg_pyramid_restore local;
    pcrcg_pyramid_restore& R = deferred ? *deferred : local;
    R.njobs = 0;
    for (int i = 0; i < nt; ++i) {
        const TableRec& t = B.tables[i];
        const RadiusSearch& s = t.s;
        const MetaView::Table m = hm.table(i);
        if (m.status() != 0) {
            set_error("pcrcg_pyramid_build: radius search capacity exceeded (table %d)", i);
            return PCRCG_ECAPACITY;
        }
        for (int p = 0; p < P; ++p) {
            // neighbors[:, :limit] keeps FEWER columns when the longest list is shorter (ref:datasets/dataloader.py:65-67)
            const int max_count = m.max_count(p);
            const int cols = max_count < s.cols ? (max_count > 0 ? max_count : 0) : s.cols;
            int row0, rows;
            group_rows(t.q_level, p, &row0, &rows);
            pcrcg_table tab{s.idx + (size_t)row0 * s.cols, rows, cols, s.cols};
            if (t.kind == 0) out[p].neighbors[t.level] = tab;
            else if (t.kind == 1) out[p].pools[t.level] = tab;
            else out[p].upsamples[t.level] = tab;
        }
        const int widest = m.widest(), tie_rows = m.tie_rows();
        if (B.want_ties && widest > 0 && tie_rows > 0 && R.njobs < PCRCG_MAX_REORDER_JOBS) {
            pcrcg_reorder_job& j = R.jobs[R.njobs++];
            const int fi = (B.one_forest || t.sup_level == 0) ? 0 : 1;
            j.q = s.q; j.qlen = s.qlen; j.rows = s.tie_rows; j.count = s.count; j.idx = s.idx;
            j.nq = level_n[t.q_level]; j.nbq = nb; j.cloud0 = B.one_forest ? t.sup_level * nb : (fi == 0 ? 0 : (t.sup_level - 1) * nb);
            j.nrows = tie_rows;
            j.max_count = widest < 8192 ? widest : 8192;   // (tieorder.hip stages at most 8192 hits per row)
            j.cols = s.cols; j.radius = s.radius; j.group = group;
            j.sup = B.level_pts[fi]; j.forest = B.forest[fi]; j.forest_ns = B.forest_ns[fi]; j.forest_nb = B.forest_nb[fi];
        }
    }
    // ---- the reference's order inside groups of exactly equal distance (tieorder.hip) ----------------------
    R.tie_status = B.tie_status;
    if (!deferred) return pcrcg_pyramid_restore_run(&R, h_status, st);
    return PCRCG_OK;
}

extern "C" {

size_t pcrcg_pyramid_ws_bytes(int n0, int nb, const pcrcg_pyramid_cfg* cfg) {
    if (!cfg || n0 < 0 || nb < 1 || cfg->n_levels < 1 || cfg->n_levels > PCRCG_MAX_LEVELS) return 0;
    Arena A(nullptr, 0, true);
    Build B;
    if (pyramid_enqueue(Parts{}, n0, nb, cfg, A, nullptr, B) != PCRCG_OK) return 0;
    return A.peak + 4096;
}

// A non-blocking HIP stream (hipStreamNonBlocking) with an optional priority (0 = default, -1 = high).
int pcrcg_stream_create(void** stream, int priority) {
    PCRCG_CHECK_ARG(stream != nullptr);
    hipStream_t st = nullptr;
    PCRCG_CHECK_HIP(hipStreamCreateWithPriority(&st, hipStreamNonBlocking, priority));
    *stream = st;
    return PCRCG_OK;
}

// cls[i] = dispatcher class of streams[i]: 0 for streams[0]'s, then 1, 2, ... in order of first appearance.  Measured, not
// looked up (the runtime does not say): a dispatch-bound kernel (2 M one-wavefront workgroups, ~0.9 ms of dispatching) on a
// class representative, a one-workgroup kernel on the candidate 150 us later, host-timed; "same dispatcher" = the tiny
// kernel took more than a third of what is left of the big dispatch.  Every candidate is tested against one representative
// per known class (at most four exist), each test twice; ~1.5 ms per test.  Call it on an otherwise idle GPU.
// scratch: >= 16 bytes of device memory.
int pcrcg_stream_pipe_classes(void* const* streams, int n, int* cls, void* scratch) {
    PCRCG_CHECK_ARG(streams && cls && scratch && n >= 1 && n <= 64);
    int* sink = static_cast<int*>(scratch);
    PCRCG_CHECK_HIP(hipDeviceSynchronize());
    for (int i = 0; i < n; ++i) hipLaunchKernelGGL(k_probe_tiny, dim3(1), dim3(64), 0, as_stream(streams[i]), sink);   // warm every queue
    PCRCG_CHECK_HIP(hipDeviceSynchronize());
    const int blocks = 2000000;
    double t0 = now_us();
    hipLaunchKernelGGL(k_probe_many, dim3(blocks), dim3(64), 0, as_stream(streams[0]), sink, 64);
    PCRCG_CHECK_HIP(hipStreamSynchronize(as_stream(streams[0])));
    const double big_us = now_us() - t0;
    if (big_us < 400.0) {      // the probe needs a dispatch that outlasts the launch of the tiny kernel
        set_error("pcrcg_stream_pipe_classes: the dispatch-bound probe kernel took only %.0f us", big_us);
        return PCRCG_ELAUNCH;
    }
    int reps[8], nrep = 0;
    auto shares = [&](int a, int b, bool* out) -> int {      // does streams[b] wait for a dispatch on streams[a]?
        // best of three, and a trial counts only if the host got from the big launch to the tiny one in time (a preempted
        // host thread finds the dispatch over and would report "another dispatcher")
        int yes = 0, no = 0;
        for (int trial = 0; trial < 10 && yes < 2 && no < 2; ++trial) {
            const double launch = now_us();
            hipLaunchKernelGGL(k_probe_many, dim3(blocks), dim3(64), 0, as_stream(streams[a]), sink, 64);
            const double start = now_us();
            while (now_us() - start < 150.0) {}
            const double a0 = now_us();
            hipLaunchKernelGGL(k_probe_tiny, dim3(1), dim3(64), 0, as_stream(streams[b]), sink);
            const double a1 = now_us();
            PCRCG_CHECK_HIP(hipStreamSynchronize(as_stream(streams[b])));
            const double d = now_us() - a0;
            PCRCG_CHECK_HIP(hipDeviceSynchronize());
            if (a1 - launch > 0.6 * big_us) continue;
            (d > (big_us - 150.0) / 3.0 ? yes : no) += 1;
        }
        if (yes < 2 && no < 2) { set_error("pcrcg_stream_pipe_classes: the host is too busy for the probe's timing"); return PCRCG_ELAUNCH; }
        *out = yes == 2;
        return PCRCG_OK;
    };
    for (int i = 0; i < n; ++i) {
        cls[i] = -1;
        for (int j = 0; j < i && cls[i] < 0; ++j)
            if (streams[j] == streams[i]) cls[i] = cls[j];
        for (int r = 0; r < nrep && cls[i] < 0; ++r) {
            bool same = false;
            PCRCG_PROPAGATE(shares(reps[r], i, &same));
            if (same) cls[i] = r;
        }
        if (cls[i] < 0) {
            if (nrep == 8) { set_error("pcrcg_stream_pipe_classes: more than 8 dispatcher classes -- the probe is not measuring what it should"); return PCRCG_ELAUNCH; }
            reps[nrep] = i;
            cls[i] = nrep++;
        }
    }
    return PCRCG_OK;
}

int pcrcg_stream_destroy(void* stream) {
    PCRCG_CHECK_HIP(hipStreamDestroy(as_stream(stream)));
    return PCRCG_OK;
}

int pcrcg_pyramid_restore_run(const pcrcg_pyramid_restore* r, int* h_status, void* stream) {
    PCRCG_CHECK_ARG(r && r->tie_status && r->njobs >= 0 && r->njobs <= PCRCG_MAX_REORDER_JOBS);
    hipStream_t st = as_stream(stream);
    if (r->njobs > 0) PCRCG_PROPAGATE(pcrcg_radius_reorder_jobs(r->jobs, r->njobs, nullptr, 0, 1, nullptr, r->tie_status, st));
    if (h_status) PCRCG_CHECK_HIP(hipMemcpyAsync(h_status, r->tie_status, sizeof(int), hipMemcpyDeviceToHost, st));
    return PCRCG_OK;
}

static int pyramid_build_checked(const Parts& in, int n0, int nb, const pcrcg_pyramid_cfg* cfg, void* ws, size_t ws_bytes,
                                 int* h_scratch, pcrcg_batch* out, int* h_lengths, int* h_status,
                                 pcrcg_pyramid_restore* deferred, void* stream) {
    PCRCG_CHECK_ARG(cfg && ws && h_scratch && out && h_lengths);
    PCRCG_CHECK_ARG(n0 >= 1 && nb >= 1 && nb <= 16);
    PCRCG_CHECK_ARG(cfg->group >= 0 && (cfg->group == 0 || nb % cfg->group == 0));
    PCRCG_CHECK_ARG((cfg->group > 0 ? nb / cfg->group : 1) + 2 <= 16 && cfg->n_levels * nb <= 64);
    PCRCG_CHECK_ARG(cfg->n_levels >= 1 && cfg->n_levels <= PCRCG_MAX_LEVELS && 3 * cfg->n_levels <= PCRCG_MAX_REORDER_JOBS);
    for (int l = 0; l < cfg->n_levels; ++l)
        PCRCG_CHECK_ARG(cfg->limit[l] >= 1 && cfg->r_conv[l] > 0.f && (l + 1 == cfg->n_levels || (cfg->dl[l] > 0.f && cfg->r_pool[l] > 0.f)));
    PCRCG_CHECK_ARG(host_scratch_ints(nb, cfg) <= kHostScratchInts);     // (implied by the checks above; kept next to them)
    Arena A(ws, ws_bytes, false);
    hipStream_t st = as_stream(stream);
    std::unique_lock<std::mutex> enqueue(*g_enqueue.of(st));
    Build B;
    int rc = pyramid_enqueue(in, n0, nb, cfg, A, st, B);
    // the ONE round trip of the call; the enqueue lock is released once the transfer is in the stream, before the wait
    if (rc == PCRCG_OK) rc = fetch(h_scratch, B.meta.w, B.meta.words(), B.lens_all, cfg->n_levels * nb, st, &enqueue);
    if (rc == PCRCG_OK) rc = pyramid_finish(B, cfg, h_scratch, out, h_lengths, h_status, deferred, st);
    if (rc == PCRCG_EWORKSPACE)
        if (A.off > ws_bytes) set_error("pcrcg_pyramid_build: arena too small (%zu needed so far, %zu given): size it with pcrcg_pyramid_ws_bytes for this cfg", A.off, ws_bytes);
    return rc;
}

int pcrcg_pyramid_build(const float* pts, int n0, const int* len, int nb, const pcrcg_pyramid_cfg* cfg, void* ws,
                        size_t ws_bytes, int* h_scratch, pcrcg_batch* out, int* h_lengths, int* h_status,
                        pcrcg_pyramid_restore* deferred, void* stream) {
    PCRCG_CHECK_ARG(pts && len);
    const Parts in{&pts, &n0, &len, &nb, 1};
    return pyramid_build_checked(in, n0, nb, cfg, ws, ws_bytes, h_scratch, out, h_lengths, h_status, deferred, stream);
}

int pcrcg_pyramid_build_parts(const float* const* pts_parts, const int* n_parts, const int* const* len_parts,
                              const int* nb_parts, int parts, const pcrcg_pyramid_cfg* cfg, void* ws, size_t ws_bytes,
                              int* h_scratch, pcrcg_batch* out, int* h_lengths, int* h_status,
                              pcrcg_pyramid_restore* deferred, void* stream) {
    PCRCG_CHECK_ARG(pts_parts && n_parts && len_parts && nb_parts && parts >= 1 && parts <= 8);
    long n0 = 0, nb = 0;
    for (int i = 0; i < parts; ++i) {
        PCRCG_CHECK_ARG(n_parts[i] >= 0 && nb_parts[i] >= 1 && len_parts[i] && (n_parts[i] == 0 || pts_parts[i]));
        n0 += n_parts[i];
        nb += nb_parts[i];
    }
    PCRCG_CHECK_ARG(n0 <= 0x7fffffffL);
    const Parts in{pts_parts, n_parts, len_parts, nb_parts, parts};
    return pyramid_build_checked(in, (int)n0, (int)nb, cfg, ws, ws_bytes, h_scratch, out, h_lengths, h_status, deferred, stream);
}
}

