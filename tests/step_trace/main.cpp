// sgcn_step_run (csrc/sgcn_step.cpp, unchanged, built with -DSGCN_STEP_TRACE) on a RECORDING back end, without a GPU.
//
//   main <program file>
//
// reads a step program and runs it; every call that sgcn_step_run makes downstream -- the library's own entry points, its
// internals and the HIP runtime -- lands in a stub that prints one line and touches nothing:
//
//   call <name> <argument> ...        integers in decimal, uint32 as u<decimal>, floats as f<8 hex digits of the bits>,
//                                     pointers, streams and events as p<decimal>; a sgcn_dropout_t* as drop(key,keep,rows,width)
//                                     or drop(null), a sgcn_plan_t* as plan(seg,nseg,fix,nfix,nslots,ws,ws_elems) or plan(null)
//   op <k> <code> <nargs> <consumed> <reads past the list>            the hook SGCN_STEP_TRACE_OP, once per executed op
//   run <i> / ret <status> / err <message>                            around every run
//
// The stubs of the extern "C" sgcn_* entries are GENERATED (tests/step_trace_cases.py, from the header as the compiler
// sees it: tests/abi_dump.py) into a second translation unit that prints through the t_* functions below.  Here are the
// hand-written ones: the sgcn:: internals sgcn_step.cpp declares, what sgcn_host.h needs (error_slot) and the twelve HIP
// functions.  Streams and events are small integers handed out in creation order (streams 101, 102, ..; events 201, ..).
// Questions whose answer decides a branch are answered from the program file's knobs, and are not printed.
//
// Program file: a text line "SGCNTRACE1 <nops> <nslots> <nknobs> <stream>", <nknobs> lines "key=value" (a key "env.NAME" is
// put into the environment instead), then <nslots> raw int64 and <nops> raw sgcn_step_op_t.
#include <hip/hip_runtime_api.h>

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../stochastic_gcn_amd/csrc/sgcn_host.h"
#include "../../stochastic_gcn_amd/csrc/sgcn_fuse.h"
#include "../../stochastic_gcn_amd/csrc/sgcn_bwd.h"
#include "../../include/sgcn.h"

namespace {
std::map<std::string, long long> knobs;
long long knob(const char* k, long long dflt) {
    auto it = knobs.find(k);
    return it == knobs.end() ? dflt : it->second;
}
uint32_t fbits(float f) {
    uint32_t b;
    std::memcpy(&b, &f, 4);
    return b;
}
int n_streams = 0, n_events = 0;
bool aux_pending = false;
thread_local char err_buf[512];
}  // namespace

// ---- the printers (the generated stubs call these) ------------------------------------------------------------------------
void t_begin(const char* name) { std::printf("call %s", name); }
void t_i(long long v) { std::printf(" %lld", v); }
void t_u(unsigned v) { std::printf(" u%u", v); }
void t_f(float v) { std::printf(" f%08x", fbits(v)); }
void t_p(const void* p) { std::printf(" p%llu", (unsigned long long)(uintptr_t)p); }
void t_drop(const void* p) {
    const sgcn_dropout_t* d = (const sgcn_dropout_t*)p;
    if (!d) { std::printf(" drop(null)"); return; }
    std::printf(" drop(u%u,f%08x,%d,%d)", d->key, fbits(d->keep), d->rows, d->width);
}
void t_plan(const void* p) {
    const sgcn_plan_t* q = (const sgcn_plan_t*)p;
    if (!q) { std::printf(" plan(null)"); return; }
    std::printf(" plan(p%llu,%lld,p%llu,%lld,%lld,p%llu,%lld)", (unsigned long long)(uintptr_t)q->dev_seg, (long long)q->nseg,
                (unsigned long long)(uintptr_t)q->dev_fix, (long long)q->nfix, (long long)q->nslots,
                (unsigned long long)(uintptr_t)q->dev_ws, (long long)q->ws_elems);
}
void t_end() { std::printf("\n"); }
long long t_rc(const char* name) { return knob((std::string("rc.") + name).c_str(), 0); }     // a generated stub's status

void sgcn_step_trace_op(int k, int op, int nargs, int pos, int overread) {
    std::printf("op %d %d %d %d %d\n", k, op, nargs, pos, overread);
}

// ---- questions answered from the knobs -----------------------------------------------------------------------------------
extern "C" int64_t sgcn_tune_get(const char* key) {
    if (!std::strcmp(key, "step_overlap")) return knob("step_overlap", 1);
    if (!std::strcmp(key, "step_fuse")) return knob("step_fuse", 127);
    return knob(key, 0);
}
extern "C" int64_t sgcn_gemm_ws_floats(int32_t, int32_t, int32_t) { return knob("gemm_ws", 0); }
extern "C" int64_t sgcn_ln_act_bwd_ws_floats(int32_t, int32_t) { return knob("ln_ws", 0); }
extern "C" int64_t sgcn_csr_transpose_ws_ints(int32_t, int64_t) { return knob("transpose_ws", 0); }

namespace sgcn {
char* error_slot() { return err_buf; }

void gemm_fwd_shape(int, int, int, int* S, int* kgroups, int* kchunk) {
    if (S) *S = (int)knob("fwd_S", 1);
    if (kgroups) *kgroups = (int)knob("fwd_kgroups", 1);
    if (kchunk) *kchunk = (int)knob("fwd_kchunk", 0);
}

static void bwd_args(int32_t n, int32_t N, int32_t K, const float* dy, int64_t lddy, const float* y, int64_t ldy,
                     const float* xhat, const float* rstd, const float* scale, int32_t relu, const float* x, int64_t ldx,
                     const float* W, int64_t ldw, float* dW, int64_t lddw, float* doffset, float* dscale, float* dx,
                     int64_t lddx, const sgcn_dropout_t* drop, float* g_tmp, float* ws, const int32_t* gidx) {
    t_i(n); t_i(N); t_i(K); t_p(dy); t_i(lddy); t_p(y); t_i(ldy); t_p(xhat); t_p(rstd); t_p(scale); t_i(relu); t_p(x); t_i(ldx);
    t_p(W); t_i(ldw); t_p(dW); t_i(lddw); t_p(doffset); t_p(dscale); t_p(dx); t_i(lddx); t_drop(drop); t_p(g_tmp); t_p(ws);
    t_p(gidx);
}
int dense_bwd_overlapped(int32_t n, int32_t N, int32_t K, const float* dy, int64_t lddy, const float* y, int64_t ldy,
                         const float* xhat, const float* rstd, const float* scale, int32_t relu, const float* x,
                         int64_t ldx, const float* W, int64_t ldw, float* dW, int64_t lddw, float* doffset,
                         float* dscale, float* dx, int64_t lddx, const sgcn_dropout_t* drop, float* g_tmp, float* ws,
                         const int32_t* gidx, void* stream) {
    t_begin("dense_bwd_overlapped");
    bwd_args(n, N, K, dy, lddy, y, ldy, xhat, rstd, scale, relu, x, ldx, W, ldw, dW, lddw, doffset, dscale, dx, lddx, drop, g_tmp, ws, gidx);
    t_p(stream); t_end();
    return (int)knob("rc.dense_bwd", 0);
}
int dense_bwd_chain(const DenseBwdArgs& u, const DenseBwdArgs& l, void* stream) {
    t_begin("dense_bwd_chain");
    bwd_args(u.n, u.N, u.K, u.dy, u.lddy, u.y, u.ldy, u.xhat, u.rstd, u.scale, u.relu, u.x, u.ldx, u.W, u.ldw, u.dW, u.lddw,
             u.doffset, u.dscale, u.dx, u.lddx, u.drop, u.g_tmp, u.ws, u.gidx);
    std::printf(" |");
    bwd_args(l.n, l.N, l.K, l.dy, l.lddy, l.y, l.ldy, l.xhat, l.rstd, l.scale, l.relu, l.x, l.ldx, l.W, l.ldw, l.dW, l.lddw,
             l.doffset, l.dscale, l.dx, l.lddx, l.drop, l.g_tmp, l.ws, l.gidx);
    t_p(stream); t_end();
    return SGCN_OK;
}
int aux_join(void* stream) {
    t_begin("aux_join"); t_p(stream); t_i(aux_pending ? 1 : 0); t_end();
    aux_pending = false;
    return SGCN_OK;
}
int aux_fork(void* stream, void** aux_stream) {
    t_begin("aux_fork"); t_p(stream); t_end();
    *aux_stream = (void*)(uintptr_t)9001;
    aux_pending = true;
    return SGCN_OK;
}
void step_mode_override(int overlap, int fuse) { t_begin("step_mode_override"); t_i(overlap); t_i(fuse); t_end(); }
int spin_launch(void* stream, int64_t usec) { t_begin("spin_launch"); t_p(stream); t_i(usec); t_end(); return SGCN_OK; }
int dw_group_begin() { t_begin("dw_group_begin"); t_end(); return SGCN_OK; }
int dw_group_flush(void* stream, bool park_reduce) {
    t_begin("dw_group_flush"); t_p(stream); t_i(park_reduce ? 1 : 0); t_end();
    return SGCN_OK;
}
int reduce_flush(void* stream) { t_begin("reduce_flush"); t_p(stream); t_end(); return SGCN_OK; }
void dw_group_abort() { t_begin("dw_group_abort"); t_end(); }
void grad_store_mode(int on) { t_begin("grad_store_mode"); t_i(on); t_end(); }
void stats_defer(int on) { t_begin("stats_defer"); t_i(on); t_end(); }
int stats_flush(void* stream) { t_begin("stats_flush"); t_p(stream); t_end(); return SGCN_OK; }
int adam_with_stats(float* theta, const float* grad, float* m, float* v, int64_t n, float lr_t, float beta1, float beta2,
                    float eps, float* avg, float decay, float one_minus, void* stream) {
    t_begin("adam_with_stats");
    t_p(theta); t_p(grad); t_p(m); t_p(v); t_i(n); t_f(lr_t); t_f(beta1); t_f(beta2); t_f(eps); t_p(avg); t_f(decay); t_f(one_minus);
    t_p(stream); t_end();
    return SGCN_OK;
}
bool scatter_park(float* H, int64_t ldh, const int32_t* idx, int32_t n, int32_t d, const float* src, int64_t lds) {
    t_begin("scatter_park"); t_p(H); t_i(ldh); t_p(idx); t_i(n); t_i(d); t_p(src); t_i(lds); t_end();
    return knob("scatter_park", 1) != 0;
}
int ce_impl(bool softmax, const float* logits, int64_t ldz, const float* labels, int64_t ldl, int32_t n, int32_t c,
            float* dlogits, int64_t lddz, float* pred, int64_t ldp, float* stats, float* rowstat, void* stream, bool overlap,
            const CeLastLayer* L) {
    t_begin("ce_impl");
    t_i(softmax ? 1 : 0); t_p(logits); t_i(ldz); t_p(labels); t_i(ldl); t_i(n); t_i(c); t_p(dlogits); t_i(lddz); t_p(pred); t_i(ldp);
    t_p(stats); t_p(rowstat); t_p(stream); t_i(overlap ? 1 : 0);
    if (!L) {
        std::printf(" last(null)");
    } else {
        std::printf(" last(");
        t_p(L->W); t_i(L->ldw); t_i(L->K);
        std::printf(" tail"); t_p(L->dx); t_i(L->lddx); t_drop(L->dx_drop);
        std::printf(" head"); t_p(L->hx); t_i(L->ldhx); t_i(L->kg); t_drop(L->h_drop);
        std::printf(" pre"); t_i(L->pre ? 1 : 0);
        if (L->pre) {
            t_p(L->px); t_i(L->ldpx); t_i(L->PK); t_p(L->PW); t_i(L->pS); t_i(L->pkchunk); t_i(L->pkg); t_drop(L->p_drop);
            t_p(L->poff); t_p(L->psc); t_f(L->peps); t_i(L->prelu); t_p(L->pY); t_i(L->ldpy); t_p(L->pxhat); t_p(L->prstd);
        }
        std::printf(" )");
    }
    t_end();
    return (int)knob("rc.ce", 0);
}
int dense_fwd_pair(int32_t M, int32_t N, int32_t K, const float* X, int64_t ldx, const float* X2, int64_t ldx2, int32_t split,
                   const float* W, int64_t ldw, const float* offset, const float* scale, float eps, int32_t relu, float* Y,
                   int64_t ldy, float* xhat, float* rstd, const sgcn_dropout_t* drop, float* ws, const int32_t* gidx,
                   const int32_t* gidx2, int32_t N2, const float* W2, int64_t ldw2, const float* offset2, const float* scale2,
                   float eps2, int32_t relu2, float* Y2, int64_t ldy2, float* xhat2, float* rstd2, const sgcn_dropout_t* drop2,
                   void* stream, int* fused) {
    t_begin("dense_fwd_pair");
    t_i(M); t_i(N); t_i(K); t_p(X); t_i(ldx); t_p(X2); t_i(ldx2); t_i(split); t_p(W); t_i(ldw); t_p(offset); t_p(scale); t_f(eps);
    t_i(relu); t_p(Y); t_i(ldy); t_p(xhat); t_p(rstd); t_drop(drop); t_p(ws); t_p(gidx); t_p(gidx2);
    std::printf(" |");
    t_i(N2); t_p(W2); t_i(ldw2); t_p(offset2); t_p(scale2); t_f(eps2); t_i(relu2); t_p(Y2); t_i(ldy2); t_p(xhat2); t_p(rstd2);
    t_drop(drop2); t_p(stream); t_end();
    *fused = (int)knob("pair_fused", 1);
    return SGCN_OK;
}
}  // namespace sgcn

// ---- the HIP runtime ---------------------------------------------------------------------------------------------------
extern "C" {
const char* hipGetErrorString(hipError_t) { return "stub"; }
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t stream) {
    t_begin("hipMemcpyAsync"); t_p(dst); t_p(src); t_i((long long)bytes); t_i((int)kind); t_p(stream); t_end();
    return hipSuccess;
}
hipError_t hipMemcpy2DAsync(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height,
                            hipMemcpyKind kind, hipStream_t stream) {
    t_begin("hipMemcpy2DAsync");
    t_p(dst); t_i((long long)dpitch); t_p(src); t_i((long long)spitch); t_i((long long)width); t_i((long long)height);
    t_i((int)kind); t_p(stream); t_end();
    return hipSuccess;
}
hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t stream) {
    t_begin("hipMemsetAsync"); t_p(dst); t_i(value); t_i((long long)bytes); t_p(stream); t_end();
    return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t* stream, unsigned int flags) {
    *stream = (hipStream_t)(uintptr_t)(101 + n_streams++);
    t_begin("hipStreamCreateWithFlags"); t_p(*stream); t_i(flags == hipStreamNonBlocking ? 1 : 0); t_end();
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t stream) { t_begin("hipStreamDestroy"); t_p(stream); t_end(); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t stream) { t_begin("hipStreamSynchronize"); t_p(stream); t_end(); return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t stream, hipEvent_t event, unsigned int flags) {
    t_begin("hipStreamWaitEvent"); t_p(stream); t_p(event); t_i(flags); t_end();
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* event, unsigned flags) {
    *event = (hipEvent_t)(uintptr_t)(201 + n_events++);
    t_begin("hipEventCreateWithFlags"); t_p(*event);
    t_i((flags & hipEventDisableTiming) ? 1 : 0); t_i((flags & hipEventDisableSystemFence) ? 1 : 0); t_end();
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t event) { t_begin("hipEventDestroy"); t_p(event); t_end(); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t event, hipStream_t stream) {
    t_begin("hipEventRecord"); t_p(event); t_p(stream); t_end();
    return hipSuccess;
}
hipError_t hipEventQuery(hipEvent_t) { return hipSuccess; }
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s <program file>\n", argv[0]); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    char line[512];
    long long nops = 0, nslots = 0, nknobs = 0, stream = 0;
    if (!std::fgets(line, sizeof line, f) || std::sscanf(line, "SGCNTRACE1 %lld %lld %lld %lld", &nops, &nslots, &nknobs, &stream) != 4 ||
        nops < 0 || nslots < 0 || nknobs < 0 || nops > (1 << 20) || nslots > (1 << 20)) {
        std::fprintf(stderr, "bad header line\n");
        return 2;
    }
    for (long long i = 0; i < nknobs; i++) {
        if (!std::fgets(line, sizeof line, f)) { std::fprintf(stderr, "short knob list\n"); return 2; }
        char* eq = std::strchr(line, '=');
        if (!eq) { std::fprintf(stderr, "bad knob line\n"); return 2; }
        *eq = 0;
        std::string val(eq + 1);
        while (!val.empty() && (val.back() == '\n' || val.back() == '\r')) val.pop_back();
        if (!std::strncmp(line, "env.", 4)) setenv(line + 4, val.c_str(), 1);
        else knobs[line] = std::strtoll(val.c_str(), nullptr, 0);
    }
    std::vector<int64_t> slots((size_t)nslots);
    std::vector<sgcn_step_op_t> ops((size_t)nops);
    if ((nslots && std::fread(slots.data(), sizeof(int64_t), (size_t)nslots, f) != (size_t)nslots) ||
        (nops && std::fread(ops.data(), sizeof(sgcn_step_op_t), (size_t)nops, f) != (size_t)nops) || std::fgetc(f) != EOF) {
        std::fprintf(stderr, "program file has the wrong length\n");
        return 2;
    }
    std::fclose(f);
    // the counts as the CALLER states them (a case may lie: slot >= nslots, nops < 0)
    const int32_t say_nops = (int32_t)knob("say_nops", nops), say_nslots = (int32_t)knob("say_nslots", nslots);
    const long long runs = knob("runs", 1);
    for (long long r = 0; r < runs; r++) {
        std::printf("run %lld\n", r);
        err_buf[0] = 0;
        const int rc = sgcn_step_run(knob("null_ops", 0) ? nullptr : ops.data(), say_nops, slots.empty() ? nullptr : slots.data(),
                                     say_nslots, (void*)(uintptr_t)stream);
        std::printf("ret %d\n", rc);
        if (rc != SGCN_OK) std::printf("err %s\n", err_buf);
    }
    return 0;
}
