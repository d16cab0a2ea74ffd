// Stand-alone driver of libsgcn's host code (sgcn_plan.cpp, sgcn_csplan.cpp, sgcn_ldsplan.cpp, sgcn_sched.cpp) for the
// sanitizer builds of tests/test_host_sanitizers.py.  Usage: driver CASEFILE BATTERY [key=value ...].
//
// It makes the library calls the product makes and prints one line per call, `name arg=value ... rc=N sum=HEX`, sum being
// FNV-1a-64 over the bytes of the call's output arrays.  tests/host_san_cases.py makes the same calls through the production
// library and expects the same lines.  Every input and output array is its own heap block of exactly the documented size
// (one byte for an empty one), so that an access one element past an end lands in a sanitizer's redzone; outputs are
// prefilled with 0xA5 so that bytes a call leaves alone hash the same everywhere.  The driver's own non-zero exit status
// means: a call failed where the battery expected success, succeeded where it expected a refusal, or an equality the
// header promises (plans independent of the thread count, the prefetcher's batches equal to the sequential loop's) broke.
#include "../../include/sgcn.h"

#include <cinttypes>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <string>
#include <vector>

static_assert(sizeof(sgcn_seg_t) == 16 && sizeof(sgcn_fix_t) == 12, "no padding: the structs hash as their fields in order");

// ---- the one stub: the tuning knobs the planners read live in sgcn_spmm.hip ------------------------------------------------
static std::map<std::string, int64_t> g_tune;
extern "C" int64_t sgcn_tune_get(const char* key) {
    auto it = g_tune.find(key ? key : "");
    return it == g_tune.end() ? -1 : it->second;
}

// ---- lines, hashes, buffers ----------------------------------------------------------------------------------------------
static int g_bad = 0;
static std::vector<std::string> g_lines;

static std::string fmt(const char* f, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof(buf), f, ap);
    va_end(ap);
    return buf;
}
static void emit(const std::string& s) {
    g_lines.push_back(s);
    puts(s.c_str());
}
static void bad(const std::string& why) {
    g_bad = 1;
    fprintf(stderr, "driver: %s\n", why.c_str());
}
static void want_ok(int rc, const char* what) {
    if (rc != 0) bad(fmt("%s returned %d: %s", what, rc, sgcn_last_error()));
}

struct Fnv {
    uint64_t h = 1469598103934665603ull;
    void add(const void* p, size_t bytes) {
        const unsigned char* b = static_cast<const unsigned char*>(p);
        for (size_t i = 0; i < bytes; i++) { h ^= b[i]; h *= 1099511628211ull; }
    }
    std::string hex() const { return fmt("%016" PRIx64, h); }
};

constexpr unsigned char kFill = 0xA5;
template <class T> struct Buf {               // an exact-size heap block (1 byte when empty), prefilled
    T* p; size_t n;
    explicit Buf(int64_t count) : n(count > 0 ? (size_t)count : 0) {
        const size_t bytes = n * sizeof(T);
        p = static_cast<T*>(malloc(bytes ? bytes : 1));
        if (!p) { fprintf(stderr, "driver: out of memory\n"); exit(3); }
        memset(static_cast<void*>(p), kFill, bytes ? bytes : 1);
    }
    ~Buf() { free(p); }
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    size_t bytes() const { return n * sizeof(T); }
    bool untouched() const {
        const unsigned char* b = reinterpret_cast<const unsigned char*>(p);
        for (size_t i = 0; i < (bytes() ? bytes() : 1); i++) if (b[i] != kFill) return false;
        return true;
    }
};
template <class T> static void add(Fnv& f, const Buf<T>& b) { f.add(b.p, b.bytes()); }

// ---- the case -------------------------------------------------------------------------------------------------------------
struct Case {
    int64_t M = 0, K = 0, nnz = 0, has_labels = 0;
    Buf<int32_t>*rowptr = nullptr, *col = nullptr, *row_group = nullptr, *col_pos = nullptr;
    Buf<float>* val = nullptr;
    bool square() const { return M == K && M > 0; }
};
static Case g_c;

template <class T> static Buf<T>* read_block(FILE* f, int64_t n) {
    Buf<T>* b = new Buf<T>(n);
    if (n > 0 && fread(b->p, sizeof(T), (size_t)n, f) != (size_t)n) { fprintf(stderr, "driver: short case file\n"); exit(3); }
    return b;
}
static void load(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "driver: cannot open %s\n", path); exit(3); }
    int64_t h[4];
    if (fread(h, 8, 4, f) != 4) { fprintf(stderr, "driver: short case file\n"); exit(3); }
    g_c.M = h[0]; g_c.K = h[1]; g_c.nnz = h[2]; g_c.has_labels = h[3];
    g_c.rowptr = read_block<int32_t>(f, g_c.M + 1);
    g_c.col = read_block<int32_t>(f, g_c.nnz);
    g_c.val = read_block<float>(f, g_c.nnz);
    if (g_c.has_labels) {
        g_c.row_group = read_block<int32_t>(f, g_c.M);
        g_c.col_pos = read_block<int32_t>(f, g_c.K);
    }
    fclose(f);
}
static void unload() { delete g_c.rowptr; delete g_c.col; delete g_c.val; delete g_c.row_group; delete g_c.col_pos; }

// ---- plan -----------------------------------------------------------------------------------------------------------------
static void battery_plan() {
    const int32_t M = (int32_t)g_c.M;
    for (int32_t T : {0, 1, 64}) {
        int64_t nseg = -1, nfix = -1, nslots = -1;
        int rc = sgcn_plan_count(g_c.rowptr->p, M, T, &nseg, &nfix, &nslots);
        want_ok(rc, "plan_count");
        emit(fmt("plan_count T=%d nseg=%" PRId64 " nfix=%" PRId64 " nslots=%" PRId64 " rc=%d sum=%s", T, nseg, nfix, nslots, rc,
                 Fnv().hex().c_str()));
        if (rc) continue;
        Buf<sgcn_seg_t> seg(nseg);
        Buf<sgcn_fix_t> fix(nfix);
        rc = sgcn_plan_fill(g_c.rowptr->p, M, T, seg.p, fix.p);
        want_ok(rc, "plan_fill");
        Fnv f; add(f, seg); add(f, fix);
        emit(fmt("plan_fill T=%d rc=%d sum=%s", T, rc, f.hex().c_str()));
    }
}

// ---- csplan ---------------------------------------------------------------------------------------------------------------
struct Warp { Buf<uint32_t>* table = nullptr; int32_t nb = 0, shift = 0; ~Warp() { delete table; } };

static void make_warp(Warp& w, int32_t max_buckets) {          // the table a plan "with the warp table" is built with
    w.table = new Buf<uint32_t>(max_buckets);
    int rc = sgcn_cs_warp_table(g_c.col->p, g_c.nnz, (int32_t)g_c.K, max_buckets, 1, 0.01, 1, w.table->p, &w.nb, &w.shift);
    want_ok(rc, "cs_warp_table");
    Fnv f; add(f, *w.table);
    emit(fmt("cs_warp_table mode=1 max_buckets=%d nbuckets=%d shift=%d rc=%d sum=%s", max_buckets, w.nb, w.shift, rc, f.hex().c_str()));
}

static void export_sized(sgcn_csbuild_t* b, int64_t rows_per_tile, std::vector<std::string>& out) {
    int64_t nt = -1, ne = -1, nfix = -1, nslots = -1;
    int32_t T_used = -1, thr = -1;
    int rc = sgcn_csbuild_sizes(b, &nt, &ne, &nfix, &nslots, &T_used, &thr);
    want_ok(rc, "csbuild_sizes");
    out.push_back(fmt("csbuild_sizes ntiles=%" PRId64 " nentries=%" PRId64 " nfix=%" PRId64 " nslots=%" PRId64 " T_used=%d rc=%d sum=%s",
                      nt, ne, nfix, nslots, T_used, rc, Fnv().hex().c_str()));
    if (rc) return;
    Buf<int64_t> tile_ptr(nt + 1);
    Buf<int32_t> colrow(ne), rows(nt * rows_per_tile), slots(nt * rows_per_tile);
    Buf<float> val(ne);
    Buf<sgcn_fix_t> fix(nfix);
    rc = sgcn_csbuild_export(b, tile_ptr.p, colrow.p, val.p, rows.p, slots.p, fix.p);
    want_ok(rc, "csbuild_export");
    Fnv f; add(f, tile_ptr); add(f, colrow); add(f, val); add(f, rows); add(f, slots); add(f, fix);
    out.push_back(fmt("csbuild_export rc=%d sum=%s", rc, f.hex().c_str()));
}

static void battery_csplan() {
    const int32_t M = (int32_t)g_c.M;
    const int32_t *rp = g_c.rowptr->p, *col = g_c.col->p;
    const float* val = g_c.val->p;
    // the two-call forms
    for (int cfg = 0; cfg < 2; cfg++) {
        const int32_t R = cfg ? 32 : 16, T = cfg ? 64 : 0;
        for (int rg = 0; rg <= (g_c.has_labels ? 1 : 0); rg++) {
            const int32_t* grp = rg ? g_c.row_group->p : nullptr;
            int64_t nt = -1, nfix = -1, nslots = -1;
            int rc = sgcn_csplan_count(rp, M, R, T, grp, &nt, &nfix, &nslots);
            want_ok(rc, "csplan_count");
            emit(fmt("csplan_count R=%d T=%d rg=%d ntiles=%" PRId64 " nfix=%" PRId64 " nslots=%" PRId64 " rc=%d sum=%s", R, T, rg, nt, nfix,
                     nslots, rc, Fnv().hex().c_str()));
            if (rc) continue;
            Buf<int64_t> tile_ptr(nt + 1);
            Buf<int32_t> colrow(g_c.nnz), rows(nt * R), slots(nt * R);
            Buf<float> vo(g_c.nnz);
            Buf<sgcn_fix_t> fix(nfix);
            rc = sgcn_csplan_fill(rp, col, val, M, R, T, grp, tile_ptr.p, colrow.p, vo.p, rows.p, slots.p, fix.p);
            want_ok(rc, "csplan_fill");
            Fnv f; add(f, tile_ptr); add(f, colrow); add(f, vo); add(f, rows); add(f, slots); add(f, fix);
            emit(fmt("csplan_fill R=%d T=%d rg=%d rc=%d sum=%s", R, T, rg, rc, f.hex().c_str()));
        }
    }
    Warp w;
    make_warp(w, 64);
    const uint32_t* wt = w.nb ? w.table->p : nullptr;
    for (int32_t G : {2, 4}) {
        for (int cfg = 0; cfg < 2; cfg++) {
            const int32_t T = cfg ? 0 : 64, rt = cfg ? 8 : 0, al = cfg ? 32 : 0;
            const uint32_t* hw = cfg ? wt : nullptr;
            int64_t nt = -1, ne = -1, nfix = -1, nslots = -1;
            int rc = sgcn_csplang_count(rp, col, M, T, rt, al, G, hw, w.shift, &nt, &ne, &nfix, &nslots);
            want_ok(rc, "csplang_count");
            emit(fmt("csplang_count G=%d T=%d round=%d align=%d warp=%d ntiles=%" PRId64 " nentries=%" PRId64 " nfix=%" PRId64 " nslots=%" PRId64
                     " rc=%d sum=%s", G, T, rt, al, hw ? 1 : 0, nt, ne, nfix, nslots, rc, Fnv().hex().c_str()));
            if (rc) continue;
            Buf<int64_t> tile_ptr(nt + 1);
            Buf<int32_t> colrow(ne), rows(nt * 16 * G), slots(nt * 16 * G);
            Buf<float> vo(ne);
            Buf<sgcn_fix_t> fix(nfix);
            rc = sgcn_csplang_fill(rp, col, val, M, T, rt, al, G, hw, w.shift, tile_ptr.p, colrow.p, vo.p, rows.p, slots.p, fix.p);
            want_ok(rc, "csplang_fill");
            Fnv f; add(f, tile_ptr); add(f, colrow); add(f, vo); add(f, rows); add(f, slots); add(f, fix);
            emit(fmt("csplang_fill G=%d T=%d round=%d align=%d warp=%d rc=%d sum=%s", G, T, rt, al, hw ? 1 : 0, rc, f.hex().c_str()));
        }
    }
    // the one-pass builder: a grid that holds every value of every setting (thinned from the full product, which took
    // minutes under ThreadSanitizer on the community graph), each plan on one thread and on one of 2, 7, 16 and "0"
    // (= SGCN_PLAN_THREADS) threads, in turn
    struct Cfg { int32_t G, T, round, align, warp, deal; };
    const Cfg grid[] = {{1, 0, 0, 0, 0, 1}, {1, 1, 8, 32, 1, 1}, {1, 64, 8, 0, 0, 0},      // (R = 32 where round_tiles is set)
                        {2, 1, 8, 32, 1, 1}, {2, 64, 0, 32, 1, 0},
                        {4, 0, 0, 0, 0, 1}, {4, 64, 8, 32, 1, 0}};
    const int32_t threads[4][2] = {{1, 2}, {1, 7}, {1, 16}, {1, 0}};
    int turn = 0;
    for (const Cfg& c : grid) {
        const int32_t G = c.G;
        for (int rg = 0; rg <= ((G == 1 && g_c.has_labels) ? 1 : 0); rg++) {
            g_tune["cs_deal"] = c.deal;
            emit(fmt("tune cs_deal=%d", c.deal));
            std::vector<std::string> first;
            for (int32_t nthr : threads[turn++ & 3]) {
                std::vector<std::string> now;
                sgcn_csbuild_t* b = nullptr;
                const int32_t R = G == 1 ? (c.round ? 32 : 16) : 16;
                int rc = sgcn_csplan_build(rp, col, val, M, G, R, c.T, c.round, c.align, rg ? g_c.row_group->p : nullptr,
                                           c.warp ? wt : nullptr, w.shift, nthr, &b);
                want_ok(rc, "csplan_build");
                now.push_back(fmt("csplan_build G=%d R=%d T=%d round=%d align=%d rg=%d warp=%d rc=%d sum=%s", G, R, c.T, c.round, c.align,
                                  rg, (c.warp && wt) ? 1 : 0, rc, Fnv().hex().c_str()));
                if (rc == 0) {
                    export_sized(b, (int64_t)R * G, now);
                    sgcn_csbuild_free(b);
                }
                for (const std::string& s : now) emit(s);
                if (first.empty()) first = now;
                else if (first != now) bad(fmt("csplan_build: the plan on %d threads differs from the plan on 1", nthr));
            }
        }
    }
}

// ---- warp -----------------------------------------------------------------------------------------------------------------
static void battery_warp() {
    for (int32_t mode : {0, 1})
        for (int32_t mb : {1, 64, 4096}) {
            std::string first;
            for (int32_t nthr : {1, 5}) {
                Buf<uint32_t> table(mb);
                int32_t nb = -1, shift = -1;
                int rc = sgcn_cs_warp_table(g_c.col->p, g_c.nnz, (int32_t)g_c.K, mb, mode, 0.01, nthr, table.p, &nb, &shift);
                want_ok(rc, "cs_warp_table");
                Fnv f; add(f, table);
                std::string s = fmt("cs_warp_table mode=%d max_buckets=%d nbuckets=%d shift=%d rc=%d sum=%s", mode, mb, nb, shift, rc, f.hex().c_str());
                emit(s);
                if (first.empty()) first = s;
                else if (first != s) bad("cs_warp_table: the table depends on the thread count");
            }
        }
}

// ---- transpose ------------------------------------------------------------------------------------------------------------
static void battery_transpose() {
    for (int with_val : {1, 0}) {
        std::string first;
        for (int32_t nthr : {1, 5}) {
            Buf<int32_t> trp(g_c.K + 1), tc(g_c.nnz);
            Buf<float> tv(with_val ? g_c.nnz : 0);
            int rc = sgcn_csr_transpose_host(g_c.rowptr->p, g_c.col->p, with_val ? g_c.val->p : nullptr, (int32_t)g_c.M, (int32_t)g_c.K, nthr,
                                             trp.p, tc.p, with_val ? tv.p : nullptr);
            want_ok(rc, "csr_transpose_host");
            Fnv f; add(f, trp); add(f, tc); add(f, tv);
            std::string s = fmt("csr_transpose_host values=%d rc=%d sum=%s", with_val, rc, f.hex().c_str());
            emit(s);
            if (first.empty()) first = s;
            else if (first != s) bad("csr_transpose_host: the result depends on the thread count");
        }
    }
}

// ---- reorder --------------------------------------------------------------------------------------------------------------
static void battery_reorder() {
    if (!g_c.square()) return;
    const int32_t n = (int32_t)g_c.M;
    const int32_t cfg[2][3] = {{0, 1, 64}, {3, 7, 1}};
    for (auto& c : cfg) {
        Buf<int32_t> comm(n);
        int32_t nc = -1;
        int rc = sgcn_reorder_lp(g_c.rowptr->p, g_c.col->p, n, c[0], (uint32_t)c[1], c[2], comm.p, &nc);
        want_ok(rc, "reorder_lp");
        Fnv f; add(f, comm);
        emit(fmt("reorder_lp max_iters=%d seed=%d min_size=%d ncomm=%d rc=%d sum=%s", c[0], c[1], c[2], nc, rc, f.hex().c_str()));
    }
}

// ---- ldsplan --------------------------------------------------------------------------------------------------------------
static void battery_ldsplan() {
    const int32_t M = (int32_t)g_c.M, K = (int32_t)g_c.K, VW = 2, NW = 8, RW = 192 / VW;
    for (int lab = 0; lab <= (g_c.has_labels ? 1 : 0); lab++)
        for (int32_t T : {0, 16})
            for (int32_t reuse : {1, 2, 3})
                for (int32_t mode : {0, 1})
                    for (int32_t ring : {80, 128}) {
                        sgcn_ldsplan_host_t* h = nullptr;
                        int rc = sgcn_ldsplan_create(g_c.rowptr->p, g_c.col->p, g_c.val->p, M, K, lab ? g_c.col_pos->p : nullptr,
                                                     lab ? g_c.row_group->p : nullptr, VW, T, reuse, mode, ring, &h);
                        want_ok(rc, "ldsplan_create");
                        emit(fmt("ldsplan_create labels=%d T=%d min_reuse=%d mode=%d ring_slots=%d rc=%d sum=%s", lab, T, reuse, mode, ring, rc,
                                 Fnv().hex().c_str()));
                        if (rc) continue;
                        Buf<int64_t> sz(19);
                        rc = sgcn_ldsplan_sizes(h, sz.p);
                        want_ok(rc, "ldsplan_sizes");
                        Fnv fs; add(fs, sz);
                        emit(fmt("ldsplan_sizes rc=%d sum=%s", rc, fs.hex().c_str()));
                        const int64_t nt = sz.p[0], nch = sz.p[1], nent = sz.p[2], nfix = sz.p[3], rnnz = sz.p[5], S = sz.p[17];
                        Buf<int32_t> tile_chunk_ptr(nt + 1), chunk_cols(nch * S), chunk_hdr(nch * NW * 32);
                        Buf<int64_t> ent_ptr(nch * NW + 1);
                        Buf<uint32_t> words(nent + 256);
                        Buf<float> vals(nent + 256), row_fold(M);
                        Buf<int32_t> tile_rows(nt * NW * RW), tile_slots(nt * NW * RW);
                        Buf<sgcn_fix_t> fix(nfix);
                        Buf<int32_t> res_rowptr(M + 1), res_col(rnnz);
                        Buf<float> res_val(rnnz);
                        rc = sgcn_ldsplan_export(h, tile_chunk_ptr.p, chunk_cols.p, chunk_hdr.p, ent_ptr.p, words.p, vals.p, row_fold.p,
                                                 tile_rows.p, tile_slots.p, fix.p, res_rowptr.p, res_col.p, res_val.p);
                        want_ok(rc, "ldsplan_export");
                        Fnv f;
                        add(f, tile_chunk_ptr); add(f, chunk_cols); add(f, chunk_hdr); add(f, ent_ptr); add(f, words); add(f, vals);
                        add(f, row_fold); add(f, tile_rows); add(f, tile_slots); add(f, fix); add(f, res_rowptr); add(f, res_col);
                        add(f, res_val);
                        emit(fmt("ldsplan_export rc=%d sum=%s", rc, f.hex().c_str()));
                        sgcn_ldsplan_destroy(h);
                    }
}

// ---- mult -----------------------------------------------------------------------------------------------------------------
static void battery_mult() {
    const int32_t n = (int32_t)(g_c.M < 1 ? 1 : (g_c.M > 300 ? 300 : g_c.M));
    Buf<float> prob(n);
    for (int32_t i = 0; i < n; i++) prob.p[i] = (float)((i * 7 + 3) % 11 + 1) / 8.0f;
    sgcn_mult_t* m = nullptr;
    int rc = sgcn_mult_create(prob.p, n, &m);
    want_ok(rc, "mult_create");
    emit(fmt("mult_create n=%d rc=%d sum=%s", n, rc, Fnv().hex().c_str()));
    if (rc) return;
    const float* bit = nullptr;
    int64_t len = -1;
    rc = sgcn_mult_tree(m, &bit, &len);
    want_ok(rc, "mult_tree");
    Fnv f; if (rc == 0) f.add(bit, (size_t)len * 4);
    emit(fmt("mult_tree len=%" PRId64 " rc=%d sum=%s", len, rc, f.hex().c_str()));
    for (float u : {0.0f, 0.125f, 0.5f, 0.875f}) {
        int32_t r = -1;
        rc = sgcn_mult_query_u(m, u, &r);
        want_ok(rc, "mult_query_u");
        emit(fmt("mult_query_u u=%.3f result=%d rc=%d sum=%s", (double)u, r, rc, Fnv().hex().c_str()));
    }
    for (int i = 0; i < (n < 5 ? n : 5); i++) {
        int32_t r = -1;
        rc = sgcn_mult_query(m, &r);
        want_ok(rc, "mult_query");
        emit(fmt("mult_query result=%d rc=%d sum=%s", r, rc, Fnv().hex().c_str()));
    }
    sgcn_mult_destroy(m);
}

// ---- sched ----------------------------------------------------------------------------------------------------------------
// The case is the graph.  Batch b of an epoch with batches of `bs` vertices is ids (b * bs + j) mod n; the labels are
// labels[i][c] = (i + c) mod 3 over two classes; two hops with degrees {2, 3}; plan_T 2 (sampled rows do get split).
constexpr int32_t kL = 2, kClasses = 2, kPlanT = 2;
static const int32_t kDegrees[kL] = {2, 3};

struct Graph {
    int32_t n; Buf<float> labels; Buf<int32_t> deg;
    Graph() : n((int32_t)g_c.M), labels((int64_t)g_c.M * kClasses), deg(kL) {
        for (int32_t i = 0; i < n; i++)
            for (int32_t c = 0; c < kClasses; c++) labels.p[(size_t)i * kClasses + c] = (float)((i + c) % 3);
        for (int l = 0; l < kL; l++) deg.p[l] = kDegrees[l];
    }
};
static Buf<int32_t>* batch_ids(int32_t n, int32_t bs, int32_t b) {
    Buf<int32_t>* ids = new Buf<int32_t>(bs);
    for (int32_t j = 0; j < bs; j++) ids->p[j] = (int32_t)(((int64_t)b * bs + j) % n);
    return ids;
}
static sgcn_sched_t* new_sampler(int cv, int is, int seed) {
    sgcn_sched_t* s = nullptr;
    int rc = sgcn_sched_create(g_c.val->p, g_c.col->p, g_c.rowptr->p, (int32_t)g_c.M, (int32_t)g_c.nnz, kL, cv, is, &s);
    want_ok(rc, "sched_create");
    emit(fmt("sched_create cv=%d is=%d rc=%d sum=%s", cv, is, rc, Fnv().hex().c_str()));
    if (rc) return nullptr;
    rc = sgcn_sched_seed(s, seed);
    want_ok(rc, "sched_seed");
    emit(fmt("sched_seed seed=%d rc=%d sum=%s", seed, rc, Fnv().hex().c_str()));
    return s;
}
// The importance sampler refuses a batch of isolated vertices ("Prob is empty") and a NaN weight: errors of the data,
// which the battery records and stops at; any other failure is the driver's.
static bool data_error(int rc) { return rc == SGCN_ERR_EMPTY_PROB || rc == SGCN_ERR_NAN; }

static std::string batch_tail(int64_t ni, int64_t nf, int rc, const Buf<int64_t>& meta, const int32_t* iw, const float* fw) {
    Fnv f;
    if (rc == 0) { add(f, meta); f.add(iw, (size_t)ni * 4); f.add(fw, (size_t)nf * 4); }
    return fmt("n_i=%" PRId64 " n_f=%" PRId64 " rc=%d sum=%s", rc == 0 ? ni : (int64_t)-1, rc == 0 ? nf : (int64_t)-1, rc, f.hex().c_str());
}

// sgcn_sched_batch_packed + _packed_copy into exact-size buffers, batch after batch: the sequence a prefetcher must deliver
static std::vector<std::string> sequential(const Graph& g, sgcn_sched_t* s, int32_t bs, int32_t nb, std::vector<int64_t>* words) {
    std::vector<std::string> tails;
    const int64_t ml = sgcn_sched_packed_meta_len(kL);
    for (int32_t b = 0; b < nb; b++) {
        Buf<int32_t>* ids = batch_ids(g.n, bs, b);
        Buf<int64_t> meta(ml);
        int64_t ni = -1, nf = -1;
        int rc = sgcn_sched_batch_packed(s, bs, ids->p, kL, g.deg.p, g.labels.p, kClasses, kPlanT, meta.p, ml, &ni, &nf);
        if (rc && !data_error(rc)) want_ok(rc, "sched_batch_packed");
        if (rc == 0) {
            Buf<int32_t> ib(ni > 0 ? ni : 1);
            Buf<float> fb(nf > 0 ? nf : 1);
            int rc2 = sgcn_sched_packed_copy(s, ib.p, fb.p);
            want_ok(rc2, "sched_packed_copy");
            tails.push_back(batch_tail(ni, nf, rc, meta, ib.p, fb.p));
            if (words) words->push_back((ni > 0 ? ni : 1) + (nf > 0 ? nf : 1));
        } else {
            tails.push_back(batch_tail(ni, nf, rc, meta, nullptr, nullptr));
        }
        emit(fmt("sched_batch_packed b=%d ", b) + tails.back());
        delete ids;
        if (rc) break;
    }
    return tails;
}

static void battery_sched() {
    if (!g_c.square()) return;
    Graph g;
    const int32_t bs = g.n < 24 ? g.n : 24, nb = 5;
    for (int novec : {0, 1}) {
        if (novec) setenv("SGCN_NO_AVX512", "1", 1); else unsetenv("SGCN_NO_AVX512");
        emit(fmt("env SGCN_NO_AVX512=%d", novec));
        for (int cv : {0, 1})
            for (int is : {0, 1}) {
                // hop by hop, every view
                sgcn_sched_t* s = new_sampler(cv, is, 3);
                if (!s) continue;
                Buf<int32_t>* ids = batch_ids(g.n, bs, 0);
                int rc = sgcn_sched_start_batch(s, bs, ids->p);
                want_ok(rc, "sched_start_batch");
                emit(fmt("sched_start_batch n=%d rc=%d sum=%s", bs, rc, Fnv().hex().c_str()));
                for (int l = 0; l < kL && rc == 0; l++) {
                    rc = sgcn_sched_expand(s, kDegrees[kL - l - 1]);
                    if (rc && !data_error(rc)) want_ok(rc, "sched_expand");
                    emit(fmt("sched_expand degree=%d rc=%d sum=%s", kDegrees[kL - l - 1], rc, Fnv().hex().c_str()));
                    if (rc) break;
                    for (int which = 0; which <= 10; which++) {
                        const int32_t* p = nullptr; int64_t len = -1;
                        int r2 = sgcn_sched_view_i32(s, which, &p, &len);
                        want_ok(r2, "sched_view_i32");
                        Fnv f; if (r2 == 0) f.add(p, (size_t)len * 4);
                        emit(fmt("sched_view_i32 which=%d len=%" PRId64 " rc=%d sum=%s", which, len, r2, f.hex().c_str()));
                    }
                    for (int which = 0; which <= 5; which++) {
                        const float* p = nullptr; int64_t len = -1;
                        int r2 = sgcn_sched_view_f32(s, which, &p, &len);
                        want_ok(r2, "sched_view_f32");
                        Fnv f; if (r2 == 0) f.add(p, (size_t)len * 4);
                        emit(fmt("sched_view_f32 which=%d len=%" PRId64 " rc=%d sum=%s", which, len, r2, f.hex().c_str()));
                    }
                }
                delete ids;
                sgcn_sched_destroy(s);
                // packed batches: a scout on the same seed tells the sizes, so that the staging buffers can be exact
                sgcn_sched_t* scout = new_sampler(cv, is, 5);
                if (!scout) continue;
                std::vector<int64_t> words;
                std::vector<std::string> want = sequential(g, scout, bs, nb, &words);
                sgcn_sched_destroy(scout);
                s = new_sampler(cv, is, 5);
                if (!s) continue;
                const int64_t ml = sgcn_sched_packed_meta_len(kL);
                for (int32_t b = 0; b < (int32_t)want.size(); b++) {
                    Buf<int32_t>* bi = batch_ids(g.n, bs, b);
                    Buf<int64_t> meta(ml);
                    int64_t ni = -1, nf = -1;
                    const bool known = b < (int32_t)words.size();
                    const bool small = known && (b & 1);
                    const int64_t cap = known ? words[(size_t)b] - (small ? 1 : 0) : 2;
                    Buf<int32_t> stage(cap);
                    rc = sgcn_sched_batch_packed_into(s, bs, bi->p, kL, g.deg.p, g.labels.p, kClasses, kPlanT, meta.p, ml, stage.p, cap, &ni, &nf);
                    std::string tail;
                    if (rc == 1) {
                        if (!small) bad("sched_batch_packed_into: a buffer of the exact size was refused");
                        if (!stage.untouched()) bad("sched_batch_packed_into: wrote into a buffer it called too small");
                        Buf<int32_t> ib(ni > 0 ? ni : 1);
                        Buf<float> fb(nf > 0 ? nf : 1);
                        int rc2 = sgcn_sched_packed_copy(s, ib.p, fb.p);
                        want_ok(rc2, "sched_packed_copy");
                        tail = batch_tail(ni, nf, 0, meta, ib.p, fb.p);
                    } else if (rc == 0) {
                        if (small) bad("sched_batch_packed_into: a buffer one word too small was accepted");
                        const int64_t n1 = ni > 0 ? ni : 1;
                        tail = batch_tail(ni, nf, 0, meta, stage.p, reinterpret_cast<const float*>(stage.p + n1));
                    } else {
                        if (!data_error(rc)) want_ok(rc, "sched_batch_packed_into");
                        tail = batch_tail(ni, nf, rc, meta, nullptr, nullptr);
                    }
                    emit(fmt("sched_batch_packed_into b=%d small=%d ret=%d ", b, small ? 1 : 0, rc) + tail);
                    if (tail != want[(size_t)b]) bad(fmt("sched_batch_packed_into: batch %d differs from sgcn_sched_batch_packed's", b));
                    delete bi;
                    if (rc < 0) break;
                }
                sgcn_sched_destroy(s);
            }
    }
    unsetenv("SGCN_NO_AVX512");
}

// ---- prefetch -------------------------------------------------------------------------------------------------------------
struct Epoch {
    int32_t n_samplers, n_packers, lag, n_slots, nb, take, cv, is;
    int64_t small_slot;          // index of the slot that holds 2 words only, -1: none
    bool compare;                // one sampler: the batches are the sequential loop's
};

static void run_epoch(const Graph& g, const Epoch& e, int32_t bs) {
    emit(fmt("epoch samplers=%d packers=%d lag=%d slots=%d batches=%d take=%d cv=%d is=%d small_slot=%" PRId64, e.n_samplers, e.n_packers, e.lag,
             e.n_slots, e.nb, e.take, e.cv, e.is, e.small_slot));
    std::vector<std::string> want;
    if (e.compare) {
        sgcn_sched_t* seq = new_sampler(e.cv, e.is, 11);
        if (!seq) return;
        want = sequential(g, seq, bs, e.nb, nullptr);
        sgcn_sched_destroy(seq);
    }
    std::vector<sgcn_sched_t*> ss;
    for (int k = 0; k < e.n_samplers; k++) {
        sgcn_sched_t* s = new_sampler(e.cv, e.is, 11 + 1000 * k);
        if (!s) return;
        ss.push_back(s);
    }
    Buf<sgcn_sched_t*> handles(e.n_samplers);
    for (int k = 0; k < e.n_samplers; k++) handles.p[k] = ss[(size_t)k];
    Buf<int32_t> ids((int64_t)e.nb * bs);
    Buf<int64_t> off(e.nb + 1);
    for (int32_t b = 0; b < e.nb; b++)
        for (int32_t j = 0; j < bs; j++) ids.p[(size_t)b * bs + j] = (int32_t)(((int64_t)b * bs + j) % g.n);
    for (int32_t b = 0; b <= e.nb; b++) off.p[b] = (int64_t)b * bs;
    std::vector<Buf<int32_t>*> slots;
    Buf<void*> ptrs(e.n_slots);
    Buf<int64_t> caps(e.n_slots);
    for (int32_t i = 0; i < e.n_slots; i++) {
        caps.p[i] = i == e.small_slot ? 2 : (1 << 20);
        slots.push_back(new Buf<int32_t>(caps.p[i]));
        ptrs.p[i] = slots.back()->p;
    }
    sgcn_prefetch_t* p = nullptr;
    int rc = sgcn_prefetch_start(handles.p, e.n_samplers, e.nb, ids.p, off.p, kL, g.deg.p, g.labels.p, kClasses, kPlanT, e.n_slots, ptrs.p, caps.p,
                                 e.lag, e.n_packers, &p);
    want_ok(rc, "prefetch_start");
    emit(fmt("prefetch_start rc=%d sum=%s", rc, Fnv().hex().c_str()));
    if (rc == 0) {
        const int64_t ml = sgcn_sched_packed_meta_len(kL);
        std::deque<int32_t> pending;
        for (int32_t b = 0; b < e.take; b++) {
            while ((int32_t)pending.size() > e.lag) {
                int r2 = sgcn_prefetch_release(p, pending.front());
                want_ok(r2, "prefetch_release");
                emit(fmt("prefetch_release rc=%d sum=%s", r2, Fnv().hex().c_str()));
                pending.pop_front();
            }
            int32_t slot = -1; int64_t ni = -1, nf = -1; const void* spill = nullptr;
            Buf<int64_t> meta(ml);
            rc = sgcn_prefetch_next(p, &slot, meta.p, &ni, &nf, &spill);
            if (rc == 1) {
                if (b < e.nb) bad(fmt("prefetch_next: the epoch ended at batch %d of %d", b, e.nb));
                emit(fmt("prefetch_next b=%d end rc=1 sum=%s", b, Fnv().hex().c_str()));
                break;
            }
            if (rc < 0) {
                if (!data_error(rc)) want_ok(rc, "prefetch_next");
                emit(fmt("prefetch_next b=%d ", b) + batch_tail(ni, nf, rc, meta, nullptr, nullptr));
                if (e.compare && (b >= (int32_t)want.size() || want[(size_t)b].find(fmt("rc=%d ", rc)) == std::string::npos))
                    bad(fmt("prefetch_next: batch %d failed, the sequential loop's did not", b));
                break;
            }
            if (slot < 0 || slot >= e.n_slots) { bad("prefetch_next: slot out of range"); break; }
            const int64_t n1 = ni > 0 ? ni : 1, need = n1 + (nf > 0 ? nf : 1);
            if ((spill != nullptr) != (need > caps.p[slot])) bad(fmt("prefetch_next: batch %d, spill and slot size disagree", b));
            const int32_t* w = spill ? static_cast<const int32_t*>(spill) : slots[(size_t)slot]->p;
            std::string tail = batch_tail(ni, nf, 0, meta, w, reinterpret_cast<const float*>(w + n1));
            emit(fmt("prefetch_next b=%d ", b) + tail);
            if (e.compare && (b >= (int32_t)want.size() || want[(size_t)b] != tail))
                bad(fmt("prefetch_next: batch %d differs from the sequential loop's", b));
            if (spill) {
                int r2 = sgcn_prefetch_release(p, slot);
                want_ok(r2, "prefetch_release");
                emit(fmt("prefetch_release rc=%d sum=%s", r2, Fnv().hex().c_str()));
            } else {
                pending.push_back(slot);
            }
        }
        Buf<double> st(4);
        int r2 = sgcn_prefetch_stats(p, st.p);
        want_ok(r2, "prefetch_stats");
        emit(fmt("prefetch_stats rc=%d sum=%s", r2, Fnv().hex().c_str()));
        sgcn_prefetch_stop(p);
        emit("prefetch_stop");
    }
    for (auto* s : ss) {               // the samplers are usable again after the stop
        Buf<int32_t>* bi = batch_ids(g.n, bs, 0);
        int r2 = sgcn_sched_start_batch(s, bs, bi->p);
        want_ok(r2, "sched_start_batch");
        delete bi;
        sgcn_sched_destroy(s);
    }
    for (auto* b : slots) delete b;
}

static void battery_prefetch() {
    if (!g_c.square()) return;
    Graph g;
    const int32_t bs = g.n < 16 ? g.n : 16, nb = 12;
    const Epoch epochs[] = {
        // samplers packers lag slots batches take cv is small compare
        {1, 0, 0, 3, nb, nb + 1, 1, 0, -1, true},      // one thread samples and packs; the whole epoch and its end
        {1, 2, 1, 6, nb, nb + 1, 1, 0, -1, true},      // a core thread and two packers
        {3, 0, 1, 8, nb, nb + 1, 1, 0, -1, false},     // three samplers
        {1, 0, 0, 3, nb, nb + 1, 1, 0, 1, true},       // slot 1 holds two words: its batches spill
        {1, 2, 1, 6, nb, nb + 1, 0, 0, 2, true},       // ... with packers (which batch meets the small slot is theirs to race for)
        {1, 0, 1, 4, nb, 4, 1, 0, -1, true},           // stop after four of twelve, producers still running
        {1, 2, 0, 5, nb, 4, 1, 0, -1, true},
        {3, 0, 0, 7, nb, 4, 0, 0, -1, false},
        {1, 0, 0, 3, 0, 1, 1, 0, -1, true},            // an epoch of no batches
        {1, 2, 0, 5, 0, 1, 1, 0, -1, true},
        {1, 0, 0, 3, nb, nb + 1, 0, 1, -1, true},      // the importance sampler: a batch of isolated vertices is an error that
        {1, 1, 0, 3, nb, nb + 1, 0, 1, -1, true},      // reaches the consumer through every producer shape
        {1, 3, 0, 7, nb, nb + 1, 0, 1, -1, true},
    };
    for (const Epoch& e : epochs) run_epoch(g, e, bs);
}

// ---- refusals -------------------------------------------------------------------------------------------------------------
// Every refusal: rc < 0, a message, no output byte written; then a call that succeeds on the same thread.
static const int32_t kTinyPtr[3] = {0, 1, 2};
static void refused(const char* what, int rc, bool clean) {
    const char* msg = sgcn_last_error();
    const int has_msg = msg && msg[0] ? 1 : 0;
    emit(fmt("refuse %s rc=%d message=%d clean=%d", what, rc, has_msg, clean ? 1 : 0));
    if (rc >= 0) bad(fmt("%s: accepted (rc %d)", what, rc));
    if (!has_msg) bad(fmt("%s: no error message", what));
    if (!clean) bad(fmt("%s: wrote to an output", what));
    int64_t a = -1, b = -1, c = -1;
    int ok = sgcn_plan_count(kTinyPtr, 2, 0, &a, &b, &c);
    want_ok(ok, "plan_count after a refusal");
    emit(fmt("plan_count nseg=%" PRId64 " nfix=%" PRId64 " nslots=%" PRId64 " rc=%d", a, b, c, ok));
}
constexpr int64_t kUnset = 0x5a5a5a5a5a5a5a5all;
static void* const kNoHandle = reinterpret_cast<void*>((uintptr_t)0x5a5a5a5a5a5a5a5aull);
template <class H> static bool handle_clean(H* h) { return h == nullptr || (void*)h == kNoHandle; }   // a refused create may null its handle

static void battery_refusals() {
    Buf<int32_t> rp(3), bad_rp(3), col(2), grp(2), neg_grp(2);
    Buf<float> val(2);
    rp.p[0] = 0; rp.p[1] = 1; rp.p[2] = 2;
    bad_rp.p[0] = 0; bad_rp.p[1] = 2; bad_rp.p[2] = 1;
    col.p[0] = 0; col.p[1] = 1; val.p[0] = 1.0f; val.p[1] = 2.0f;
    grp.p[0] = 0; grp.p[1] = 0; neg_grp.p[0] = 0; neg_grp.p[1] = -1;
    Buf<uint32_t> warp(4);
    for (int i = 0; i < 4; i++) warp.p[i] = 0;
    int64_t a, b, c, d;
    auto unset = [&] { a = b = c = d = kUnset; };
    auto all_unset = [&] { return a == kUnset && b == kUnset && c == kUnset && d == kUnset; };
    int rc;

    // negative M
    unset(); rc = sgcn_plan_count(rp.p, -1, 0, &a, &b, &c); refused("plan_count M=-1", rc, all_unset());
    { Buf<sgcn_seg_t> seg(2); Buf<sgcn_fix_t> fix(1);
      rc = sgcn_plan_fill(rp.p, -1, 0, seg.p, fix.p); refused("plan_fill M=-1", rc, seg.untouched() && fix.untouched()); }
    unset(); rc = sgcn_csplan_count(rp.p, -1, 16, 0, nullptr, &a, &b, &c); refused("csplan_count M=-1", rc, all_unset());
    unset(); rc = sgcn_csplang_count(rp.p, col.p, -1, 0, 0, 0, 2, nullptr, 0, &a, &b, &c, &d); refused("csplang_count M=-1", rc, all_unset());
    { sgcn_csbuild_t* h = (sgcn_csbuild_t*)kNoHandle;
      rc = sgcn_csplan_build(rp.p, col.p, val.p, -1, 1, 16, 0, 0, 0, nullptr, nullptr, 0, 1, &h); refused("csplan_build M=-1", rc, handle_clean(h)); }
    { sgcn_ldsplan_host_t* h = (sgcn_ldsplan_host_t*)kNoHandle;
      rc = sgcn_ldsplan_create(rp.p, col.p, val.p, -1, 2, nullptr, nullptr, 2, 0, 1, 0, 0, &h); refused("ldsplan_create M=-1", rc, handle_clean(h)); }
    { Buf<int32_t> trp(3), tc(2); Buf<float> tv(2);
      rc = sgcn_csr_transpose_host(rp.p, col.p, val.p, -1, 2, 1, trp.p, tc.p, tv.p);
      refused("csr_transpose_host M=-1", rc, trp.untouched() && tc.untouched() && tv.untouched()); }
    { Buf<int32_t> comm(2); int32_t nc = 0x5a5a5a5a;
      rc = sgcn_reorder_lp(rp.p, col.p, -1, 0, 1, 1, comm.p, &nc); refused("reorder_lp n=-1", rc, comm.untouched() && nc == 0x5a5a5a5a); }
    { sgcn_sched_t* h = (sgcn_sched_t*)kNoHandle;
      rc = sgcn_sched_create(val.p, col.p, rp.p, -1, 2, 1, 0, 0, &h); refused("sched_create num_data=-1", rc, handle_clean(h)); }

    // a row pointer that goes down
    unset(); rc = sgcn_plan_count(bad_rp.p, 2, 0, &a, &b, &c); refused("plan_count rowptr", rc, all_unset());
    { Buf<sgcn_seg_t> seg(2); Buf<sgcn_fix_t> fix(1);
      rc = sgcn_plan_fill(bad_rp.p, 2, 0, seg.p, fix.p); refused("plan_fill rowptr", rc, seg.untouched() && fix.untouched()); }
    unset(); rc = sgcn_csplan_count(bad_rp.p, 2, 16, 0, nullptr, &a, &b, &c); refused("csplan_count rowptr", rc, all_unset());
    { sgcn_csbuild_t* h = (sgcn_csbuild_t*)kNoHandle;
      rc = sgcn_csplan_build(bad_rp.p, col.p, val.p, 2, 1, 16, 0, 0, 0, nullptr, nullptr, 0, 1, &h); refused("csplan_build rowptr", rc, handle_clean(h)); }
    { sgcn_csbuild_t* h = (sgcn_csbuild_t*)kNoHandle;
      rc = sgcn_csplan_build(bad_rp.p, col.p, val.p, 2, 2, 16, 0, 0, 0, nullptr, nullptr, 0, 1, &h); refused("csplan_build G=2 rowptr", rc, handle_clean(h)); }
    { sgcn_ldsplan_host_t* h = (sgcn_ldsplan_host_t*)kNoHandle;
      rc = sgcn_ldsplan_create(bad_rp.p, col.p, val.p, 2, 2, nullptr, nullptr, 2, 0, 1, 0, 0, &h); refused("ldsplan_create rowptr", rc, handle_clean(h)); }

    // a column id that does not fit the packed word: 2^28 (16-row tiles), 2^27 (32-row tiles); one below is a plan
    for (int form = 0; form < 4; form++) {            // csplan_fill R=16, R=32, csplang_fill G=2, G=4
        const int32_t R = form == 1 ? 32 : 16, G = form < 2 ? 1 : (form == 2 ? 2 : 4);
        const int32_t limit = R == 32 ? (1 << 27) : (1 << 28);
        for (int over = 1; over >= 0; over--) {
            Buf<int32_t> c1(2);
            c1.p[0] = 3; c1.p[1] = over ? limit : limit - 1;
            int64_t nt = -1, ne = 2, nf = 0, ns = 0;
            if (G == 1) want_ok(sgcn_csplan_count(rp.p, 2, R, 0, nullptr, &nt, &nf, &ns), "csplan_count");
            else want_ok(sgcn_csplang_count(rp.p, over ? col.p : c1.p, 2, 0, 0, 0, G, nullptr, 0, &nt, &ne, &nf, &ns), "csplang_count");
            Buf<int64_t> tp(nt + 1);
            Buf<int32_t> cr(ne), rows(nt * R * G), slots(nt * R * G);
            Buf<float> vo(ne);
            Buf<sgcn_fix_t> fix(nf);
            rc = G == 1 ? sgcn_csplan_fill(rp.p, c1.p, val.p, 2, R, 0, nullptr, tp.p, cr.p, vo.p, rows.p, slots.p, fix.p)
                        : sgcn_csplang_fill(rp.p, c1.p, val.p, 2, 0, 0, 0, G, nullptr, 0, tp.p, cr.p, vo.p, rows.p, slots.p, fix.p);
            const std::string what = fmt("%s R=%d G=%d col=2^%d%s", G == 1 ? "csplan_fill" : "csplang_fill", R, G, R == 32 ? 27 : 28, over ? "" : "-1");
            if (over) {
                refused(what.c_str(), rc, tp.untouched() && cr.untouched() && vo.untouched() && rows.untouched() && slots.untouched());
            } else {
                want_ok(rc, what.c_str());
                Fnv f; add(f, tp); add(f, cr); add(f, vo); add(f, rows); add(f, slots); add(f, fix);
                emit(fmt("accept %s rc=%d sum=%s", what.c_str(), rc, f.hex().c_str()));
            }
        }
    }

    // a negative group label
    unset(); rc = sgcn_csplan_count(rp.p, 2, 16, 0, neg_grp.p, &a, &b, &c); refused("csplan_count group=-1", rc, all_unset());
    { sgcn_csbuild_t* h = (sgcn_csbuild_t*)kNoHandle;
      rc = sgcn_csplan_build(rp.p, col.p, val.p, 2, 1, 16, 0, 0, 0, neg_grp.p, nullptr, 0, 1, &h); refused("csplan_build group=-1", rc, handle_clean(h)); }
    { sgcn_ldsplan_host_t* h = (sgcn_ldsplan_host_t*)kNoHandle;
      rc = sgcn_ldsplan_create(rp.p, col.p, val.p, 2, 2, nullptr, neg_grp.p, 2, 0, 1, 0, 0, &h); refused("ldsplan_create group=-1", rc, handle_clean(h)); }
    { sgcn_csbuild_t* h = (sgcn_csbuild_t*)kNoHandle;        // lane-group plans are ungrouped
      rc = sgcn_csplan_build(rp.p, col.p, val.p, 2, 2, 16, 0, 0, 0, grp.p, nullptr, 0, 1, &h); refused("csplan_build G=2 grouped", rc, handle_clean(h)); }

    // warp_shift 28
    unset(); rc = sgcn_csplang_count(rp.p, col.p, 2, 0, 0, 0, 2, warp.p, 28, &a, &b, &c, &d); refused("csplang_count warp_shift=28", rc, all_unset());
    { sgcn_csbuild_t* h = (sgcn_csbuild_t*)kNoHandle;
      rc = sgcn_csplan_build(rp.p, col.p, val.p, 2, 2, 16, 0, 0, 0, nullptr, warp.p, 28, 1, &h); refused("csplan_build warp_shift=28", rc, handle_clean(h)); }

    // three lane groups
    unset(); rc = sgcn_csplang_count(rp.p, col.p, 2, 0, 0, 0, 3, nullptr, 0, &a, &b, &c, &d); refused("csplang_count ngroups=3", rc, all_unset());
    { Buf<int64_t> tp(2); Buf<int32_t> cr(128), rows(48), slots(48); Buf<float> vo(128); Buf<sgcn_fix_t> fix(0);
      rc = sgcn_csplang_fill(rp.p, col.p, val.p, 2, 0, 0, 0, 3, nullptr, 0, tp.p, cr.p, vo.p, rows.p, slots.p, fix.p);
      refused("csplang_fill ngroups=3", rc, tp.untouched() && cr.untouched() && vo.untouched() && rows.untouched() && slots.untouched()); }
    { sgcn_csbuild_t* h = (sgcn_csbuild_t*)kNoHandle;
      rc = sgcn_csplan_build(rp.p, col.p, val.p, 2, 3, 16, 0, 0, 0, nullptr, nullptr, 0, 1, &h); refused("csplan_build ngroups=3", rc, handle_clean(h)); }
    { sgcn_csbuild_t* h = (sgcn_csbuild_t*)kNoHandle;
      rc = sgcn_csplan_build(rp.p, col.p, val.p, 2, 1, 33, 0, 0, 0, nullptr, nullptr, 0, 1, &h); refused("csplan_build R=33", rc, handle_clean(h)); }

    // null required pointers
    unset(); rc = sgcn_plan_count(nullptr, 2, 0, &a, &b, &c); refused("plan_count rowptr=null", rc, all_unset());
    unset(); rc = sgcn_plan_count(rp.p, 2, 0, &a, nullptr, &c); refused("plan_count nfix=null", rc, all_unset());
    rc = sgcn_plan_fill(rp.p, 2, 0, nullptr, nullptr); refused("plan_fill seg=null", rc, true);
    { Buf<int32_t> wide(3); Buf<sgcn_seg_t> seg(3);          // a row of two nonzeros at T = 1 is split: it needs a fix array
      wide.p[0] = 0; wide.p[1] = 2; wide.p[2] = 3;
      rc = sgcn_plan_fill(wide.p, 2, 1, seg.p, nullptr); refused("plan_fill fix=null", rc, seg.untouched()); }
    unset(); rc = sgcn_csplan_count(rp.p, 2, 16, 0, nullptr, nullptr, &b, &c); refused("csplan_count ntiles=null", rc, all_unset());
    rc = sgcn_csplan_build(rp.p, col.p, val.p, 2, 1, 16, 0, 0, 0, nullptr, nullptr, 0, 1, nullptr); refused("csplan_build out=null", rc, true);
    { sgcn_csbuild_t* h = (sgcn_csbuild_t*)kNoHandle;
      rc = sgcn_csplan_build(rp.p, nullptr, val.p, 2, 1, 16, 0, 0, 0, nullptr, nullptr, 0, 1, &h); refused("csplan_build col=null", rc, handle_clean(h)); }
    unset(); rc = sgcn_csbuild_sizes(nullptr, &a, &b, &c, &d, nullptr, nullptr); refused("csbuild_sizes b=null", rc, all_unset());
    rc = sgcn_csbuild_export(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr); refused("csbuild_export b=null", rc, true);
    { sgcn_csbuild_t* h = nullptr;
      want_ok(sgcn_csplan_build(rp.p, col.p, val.p, 2, 1, 16, 0, 0, 0, nullptr, nullptr, 0, 1, &h), "csplan_build");
      Buf<int32_t> cr(2); Buf<float> vo(2);
      rc = sgcn_csbuild_export(h, nullptr, cr.p, vo.p, nullptr, nullptr, nullptr); refused("csbuild_export tile_ptr=null", rc, cr.untouched() && vo.untouched());
      sgcn_csbuild_free(h); }
    { Buf<uint32_t> table(4); int32_t sh = 0x5a5a5a5a;
      rc = sgcn_cs_warp_table(col.p, 2, 2, 4, 1, 0.01, 1, table.p, nullptr, &sh); refused("cs_warp_table nbuckets=null", rc, table.untouched() && sh == 0x5a5a5a5a); }
    { Buf<int32_t> tc(2); Buf<float> tv(2);
      rc = sgcn_csr_transpose_host(rp.p, col.p, val.p, 2, 2, 1, nullptr, tc.p, tv.p); refused("csr_transpose_host t_rowptr=null", rc, tc.untouched() && tv.untouched()); }
    rc = sgcn_sched_create(val.p, col.p, rp.p, 2, 2, 1, 0, 0, nullptr); refused("sched_create out=null", rc, true);
    rc = sgcn_mult_create(val.p, 2, nullptr); refused("mult_create out=null", rc, true);
    rc = sgcn_ldsplan_create(rp.p, col.p, val.p, 2, 2, nullptr, nullptr, 2, 0, 1, 0, 0, nullptr); refused("ldsplan_create out=null", rc, true);
    { Buf<int64_t> sz(19); rc = sgcn_ldsplan_sizes(nullptr, sz.p); refused("ldsplan_sizes h=null", rc, sz.untouched()); }
    { sgcn_ldsplan_host_t* h = (sgcn_ldsplan_host_t*)kNoHandle;
      rc = sgcn_ldsplan_create(rp.p, col.p, val.p, 2, 2, nullptr, nullptr, 4, 0, 1, 0, 0, &h); refused("ldsplan_create VW=4", rc, handle_clean(h)); }
    { sgcn_ldsplan_host_t* h = (sgcn_ldsplan_host_t*)kNoHandle;
      rc = sgcn_ldsplan_create(rp.p, col.p, val.p, 2, 2, nullptr, nullptr, 2, 0, 1, 0, 96, &h); refused("ldsplan_create ring_slots=96", rc, handle_clean(h)); }
    { sgcn_ldsplan_host_t* h = (sgcn_ldsplan_host_t*)kNoHandle;
      Buf<int32_t> pos(2); pos.p[0] = 1; pos.p[1] = 1;
      rc = sgcn_ldsplan_create(rp.p, col.p, val.p, 2, 2, pos.p, nullptr, 2, 0, 1, 0, 0, &h); refused("ldsplan_create col_pos repeated", rc, handle_clean(h)); }
    { sgcn_ldsplan_host_t* h = (sgcn_ldsplan_host_t*)kNoHandle;
      rc = sgcn_ldsplan_create(rp.p, col.p, val.p, 2, 1, nullptr, nullptr, 2, 0, 1, 0, 0, &h); refused("ldsplan_create col>=K", rc, handle_clean(h)); }

    // max_buckets 0
    { Buf<uint32_t> table(4); int32_t nb = 0x5a5a5a5a, sh = 0x5a5a5a5a;
      rc = sgcn_cs_warp_table(col.p, 2, 2, 0, 1, 0.01, 1, table.p, &nb, &sh);
      refused("cs_warp_table max_buckets=0", rc, table.untouched() && nb == 0x5a5a5a5a && sh == 0x5a5a5a5a); }
    // a column outside [0, K): the histogram and the transpose
    { Buf<uint32_t> table(4); int32_t nb = 0x5a5a5a5a, sh = 0x5a5a5a5a;
      rc = sgcn_cs_warp_table(col.p, 2, 1, 4, 1, 0.01, 1, table.p, &nb, &sh); refused("cs_warp_table col>=K", rc, table.untouched()); }
    { Buf<int32_t> trp(2), tc(2); Buf<float> tv(2);
      rc = sgcn_csr_transpose_host(rp.p, col.p, val.p, 2, 1, 1, trp.p, tc.p, tv.p);
      refused("csr_transpose_host col>=K", rc, trp.untouched() && tc.untouched() && tv.untouched()); }

    // an empty probability vector
    { sgcn_mult_t* h = (sgcn_mult_t*)kNoHandle;
      rc = sgcn_mult_create(val.p, 0, &h); refused("mult_create n=0", rc, handle_clean(h));
      if (rc != SGCN_ERR_EMPTY_PROB) bad("mult_create n=0: not SGCN_ERR_EMPTY_PROB"); }

    // a descriptor table one short
    { sgcn_sched_t* s = nullptr;
      want_ok(sgcn_sched_create(val.p, col.p, rp.p, 2, 2, 1, 1, 0, &s), "sched_create");
      const int64_t ml = sgcn_sched_packed_meta_len(1);
      Buf<int64_t> meta(ml - 1);
      Buf<float> lab(4);
      for (int i = 0; i < 4; i++) lab.p[i] = (float)i;
      Buf<int32_t> ids(2), deg(1);
      ids.p[0] = 0; ids.p[1] = 1; deg.p[0] = 1;
      unset(); rc = sgcn_sched_batch_packed(s, 2, ids.p, 1, deg.p, lab.p, 2, 0, meta.p, ml - 1, &a, &b);
      refused("sched_batch_packed meta_cap-1", rc, meta.untouched() && a == kUnset && b == kUnset);
      Buf<int32_t> stage(64);
      unset(); rc = sgcn_sched_batch_packed_into(s, 2, ids.p, 1, deg.p, lab.p, 2, 0, meta.p, ml - 1, stage.p, 64, &a, &b);
      refused("sched_batch_packed_into meta_cap-1", rc, meta.untouched() && stage.untouched() && a == kUnset && b == kUnset);
      { const int32_t* p = nullptr; int64_t len = kUnset;
        rc = sgcn_sched_view_i32(s, 11, &p, &len); refused("sched_view_i32 which=11", rc, p == nullptr && len == kUnset);
        const float* q = nullptr; len = kUnset;
        rc = sgcn_sched_view_f32(s, 6, &q, &len); refused("sched_view_f32 which=6", rc, q == nullptr && len == kUnset); }
      // the prefetcher's argument errors
      { sgcn_prefetch_t* p = (sgcn_prefetch_t*)kNoHandle;
        Buf<int64_t> off(2), caps(2); Buf<void*> ptrs(2); Buf<int32_t> w0(8), w1(8);
        off.p[0] = 0; off.p[1] = 2; caps.p[0] = caps.p[1] = 8; ptrs.p[0] = w0.p; ptrs.p[1] = w1.p;
        sgcn_sched_t* one[1] = {s};
        rc = sgcn_prefetch_start(nullptr, 1, 1, ids.p, off.p, 1, deg.p, lab.p, 2, 0, 2, ptrs.p, caps.p, 0, 0, &p);
        refused("prefetch_start samplers=null", rc, handle_clean(p));
        p = (sgcn_prefetch_t*)kNoHandle;
        rc = sgcn_prefetch_start(one, 1, 1, ids.p, off.p, 1, deg.p, lab.p, 2, 0, 2, ptrs.p, caps.p, 1, 0, &p);
        refused("prefetch_start lag+1>=n_slots", rc, handle_clean(p));
        sgcn_sched_t* two[2] = {s, s};
        p = (sgcn_prefetch_t*)kNoHandle;
        rc = sgcn_prefetch_start(two, 2, 1, ids.p, off.p, 1, deg.p, lab.p, 2, 0, 2, ptrs.p, caps.p, 0, 1, &p);
        refused("prefetch_start packers with two samplers", rc, handle_clean(p));
        rc = sgcn_prefetch_release(nullptr, 0); refused("prefetch_release p=null", rc, true); }
      // and the sampler still works
      Buf<int64_t> full(ml);
      want_ok(sgcn_sched_batch_packed(s, 2, ids.p, 1, deg.p, lab.p, 2, 0, full.p, ml, &a, &b), "sched_batch_packed");
      sgcn_sched_destroy(s); }
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s CASEFILE BATTERY [key=value ...]\n", argv[0]); return 2; }
    for (int i = 3; i < argc; i++) {
        const char* eq = strchr(argv[i], '=');
        if (!eq) { fprintf(stderr, "driver: %s is not key=value\n", argv[i]); return 2; }
        g_tune[std::string(argv[i], (size_t)(eq - argv[i]))] =strtoll(eq + 1, nullptr, 10);
    }
    setenv("SGCN_PLAN_THREADS", "8", 1);        // what a call with nthreads = 0 uses
    load(argv[1]);
    const std::string b = argv[2];
    if (b == "plan") battery_plan();
    else if (b == "csplan") battery_csplan();
    else if (b == "warp") battery_warp();
    else if (b == "transpose") battery_transpose();
    else if (b == "reorder") battery_reorder();
    else if (b == "ldsplan") battery_ldsplan();
    else if (b == "mult") battery_mult();
    else if (b == "sched") battery_sched();
    else if (b == "prefetch") battery_prefetch();
    else if (b == "refusals") battery_refusals();
    else { fprintf(stderr, "driver: no battery %s\n", b.c_str()); unload(); return 2; }
    unload();
    fflush(stdout);
    return g_bad;
}
