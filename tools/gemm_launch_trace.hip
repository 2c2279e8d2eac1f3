// gemm_launch_trace.hip -- the launches of the GEMM path, traced on the host: for a table of problems, qoc_gemm_setup, qoc_gemm_lds_opt_in and two
// iterations of qoc_gemm_expm / qoc_gemm_forward / qoc_gemm_backward (the backward pass both with and without "the tail sums the partials"), the
// read-back form of the forward pass where final_state is formed lazily, the time-sharded evaluation with an emulating rank where it applies, then
// teardown -- all through the shim launch_trace.h.  A host-side edit is checked by building this program against csrc/ before and after it and
// comparing the two outputs:
//
//   hipcc --offload-arch=gfx950 -O1 -std=c++17 -Wno-unused-value -rdynamic -DQOC_TRACE_STREAMS -include tools/launch_trace.h -I <csrc> -I include \
//       tools/gemm_launch_trace.hip <csrc>/qoc_gemm_wg.hip -o gemm_launch_trace -ldl
//   ./gemm_launch_trace > after.txt          one line per problem: its parameters, the number of trace lines, a hash of them; then the kernels reached
//   ./gemm_launch_trace -v 1 > after_v.txt   the trace lines themselves for every problem (-v <j>: every j-th), -o <i>: of problem i alone
//   ./gemm_launch_trace -f rows.txt          the problems of a file (fourteen integers per line, see main) instead of the table
//
// A trace line is a launch (kernel symbol from dladdr, stream, grid, block, dynamic LDS, the integer arguments, the pointer arguments by allocation
// and offset, the structs word by word: an 8-byte word that points into a traced allocation as a<i>+<offset>, anything else as hex), an event record /
// wait, a memset, a stream / event creation or destruction, an allocation, or -- not hashed, -v only -- an LDS reservation.  Streams and events are
// numbered in creation order; the engine's stream is 0.  Needs no GPU; not part of build().
#include <dlfcn.h>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>
#include "qoc_common.h"
#include "qoc_kernels_finish.h"
#include "qoc_kernels_generic.h"
#include "qoc_kernels_mfma.h"
#include "qoc_kernels_st.h"
#include "qoc_kernels_gemm.h"
#include "qoc_gemm_ts.h"

// csrc/ with the route kept in QocGemm (qoc_gemm_routes.h) or with the two booleans before it
#if __has_include("qoc_gemm_routes.h")
#define ROUTE_NAME(gm) ((gm).route == QOC_GEMM_DIRECT ? "direct" : (gm).route == QOC_GEMM_PERSISTENT ? "persistent" : "stepwise")
#define BACKWARD(gm, d, s, tail_sums) qoc_gemm_backward(gm, d, s, tail_sums)
#else
#define ROUTE_NAME(gm) ((gm).direct ? "direct" : (gm).persistent ? "persistent" : "stepwise")
#define BACKWARD(gm, d, s, tail_sums) ((gm).reduce_in_tail = (tail_sums), qoc_gemm_backward(gm, d, s))
#endif

// (a time-sharded engine's collectives: an emulating rank never calls them)
void qoc_comm_detach(qoc_comm*) {}
int qoc_ts_all_gather(qoc_comm*, void*, size_t, hipStream_t) { return 0; }
int qoc_ts_all_reduce_sum(qoc_comm*, double*, size_t, hipStream_t) { return 0; }

struct Alloc { char* p; size_t bytes; };
static std::vector<Alloc> g_allocs;                    // of the current problem, in allocation order
static std::set<std::string> g_kernels;
static std::string g_text;                             // the current problem's trace
static unsigned long long g_hash;
static long g_lines;
static bool g_verbose;
static int g_streams, g_events;                        // handles made so far for the current problem (handle = number, as a pointer)

static void line(bool hashed, const char* fmt, ...) {
    char buf[8192];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (hashed) { for (const char* c = buf; *c; ++c) g_hash = (g_hash ^ (unsigned char)*c) * 1099511628211ull; ++g_lines; }
    if (g_verbose) { g_text += buf; g_text += '\n'; }
}
static std::string symbol(const void* f) {
    Dl_info info;
    return dladdr(f, &info) && info.dli_sname ? info.dli_sname : "?";
}
// a<i>+<offset> for a pointer into (or one past) a traced allocation, else ""
static std::string traced(const void* p) {
    for (size_t a = 0; a < g_allocs.size(); ++a)
        if ((const char*)p >= g_allocs[a].p && (const char*)p < g_allocs[a].p + g_allocs[a].bytes) {
            char buf[64];
            snprintf(buf, sizeof buf, "a%zu+%zu", a, (size_t)((const char*)p - g_allocs[a].p));
            return buf;
        }
    return "";
}
static std::string pointer(const void* p) {
    if (!p) return "null";
    const std::string t = traced(p);
    if (!t.empty()) return t;
    // (a chain that runs backwards starts a step before or behind its buffer: by distance from the nearest allocation)
    for (size_t a = 0; a < g_allocs.size(); ++a) {
        const long long off = (const char*)p - g_allocs[a].p;
        if (off > -(1ll << 24) && off < (long long)g_allocs[a].bytes + (1ll << 24)) { char buf[64]; snprintf(buf, sizeof buf, "a%zu%+lld", a, off); return buf; }
    }
    return "stray";
}
static std::string words(const void* p, size_t size) {
    std::string s = " {";
    char buf[64];
    size_t o = 0;
    for (; o + 8 <= size; o += 8) {
        unsigned long long w;
        memcpy(&w, (const char*)p + o, 8);
        const std::string t = w ? traced((const void*)w) : std::string();
        if (!t.empty()) s += t; else { snprintf(buf, sizeof buf, "%llx", w); s += buf; }
        s += o + 8 < size ? " " : "";
    }
    if (o < size) { unsigned long long w = 0; memcpy(&w, (const char*)p + o, size - o); snprintf(buf, sizeof buf, "%llx", w); s += buf; }
    return s + "}";
}
static int number(const void* handle) { return (int)(size_t)handle; }

hipError_t qoc_trace_malloc(void** p, size_t bytes) {
    *p = calloc(1, bytes ? bytes : 1);
    if (!*p) return hipErrorOutOfMemory;
    g_allocs.push_back({(char*)*p, bytes});
    line(true, "  alloc a%zu %zu", g_allocs.size() - 1, bytes);
    return hipSuccess;
}
hipError_t qoc_trace_reserve(const void* kernel, int bytes) {
    line(false, "  reserve %s %d", symbol(kernel).c_str(), bytes);
    return hipSuccess;
}
hipError_t qoc_trace_launch(const void* kernel, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const QocTraceArg* args, int count) {
    const std::string name = symbol(kernel);
    g_kernels.insert(name);
    std::string a;
    char buf[64];
    for (int i = 0; i < count; ++i) {
        const QocTraceArg& x = args[i];
        if (x.kind == QocTraceArg::INT) { snprintf(buf, sizeof buf, " %lld", x.i); a += buf; }
        else if (x.kind == QocTraceArg::PTR) a += " " + pointer(x.p);
        else a += words(x.p, x.size);
    }
    line(true, "  launch %s stream=%d grid=%u,%u,%u block=%u,%u,%u lds=%zu%s", name.c_str(), number(stream), grid.x, grid.y, grid.z, block.x, block.y, block.z, lds,
         a.c_str());
    return hipSuccess;
}
hipError_t qoc_trace_stream_create(hipStream_t* s, unsigned nwords, const uint32_t* mask) {
    *s = (hipStream_t)(size_t)++g_streams;
    std::string m;
    char buf[32];
    for (unsigned i = 0; i < nwords; ++i) { snprintf(buf, sizeof buf, " %08x", mask[i]); m += buf; }
    line(true, "  stream %d%s%s", g_streams, nwords ? " cu_mask" : "", m.c_str());
    return hipSuccess;
}
hipError_t qoc_trace_event_create(hipEvent_t* e) {
    *e = (hipEvent_t)(size_t)++g_events;
    line(true, "  event %d", g_events);
    return hipSuccess;
}
hipError_t qoc_trace_destroy(const char* what, const void* handle) {
    line(true, "  destroy %s %d", what, number(handle));
    return hipSuccess;
}
hipError_t qoc_trace_event(const char* what, hipEvent_t e, hipStream_t s) {
    line(true, "  %s event=%d stream=%d", what, number(e), number(s));
    return hipSuccess;
}
hipError_t qoc_trace_memset(void* p, int value, size_t bytes, hipStream_t s, bool async) {
    line(true, "  memset%s %s value=%d bytes=%zu stream=%d", async ? "_async" : "", pointer(p).c_str(), value, bytes, number(s));
    memset(p, value, bytes);
    return hipSuccess;
}

// reg: 0 none, 1 forbidden levels, 2 speed_up.  variant: qoc_config.variant of an explicit GEMM-path request.  direct: AUTO's (or the caller's) wish for the
// direct route.  G: time shards (0: none).  sw / sw2: experimental switches set around set-up
struct Problem { int n, k, m, T, s, st, reg, variant, direct, antiherm, B, Bplan, steps, G; const char* sw; const char* sw_value; const char* sw2; const char* sw2_value; };
static const char* const SWITCHES[] = {"QOC_CHAIN_DPP", "QOC_DPP_ACTIVE_COLUMNS", "QOC_ASM_OVERLAP", "QOC_ASM_CUMASK", "QOC_ASM_TAIL_WGS", "QOC_ASM_SPLIT16", "QOC_ASM_WINDOWS"};

template <class T> static T* dev(std::vector<void*>& owned, size_t count) {
    void* p = nullptr;
    (void)hipMalloc(&p, (count ? count : 1) * sizeof(T));
    owned.push_back(p);
    return (T*)p;
}

static void gm_digest(const QocGemm& gm) {
    std::string win;
    char buf[32];
    for (int w : gm.asm_win) { snprintf(buf, sizeof buf, " %d", w); win += buf; }
    std::string tree;
    for (int l = 1; l <= gm.L; ++l) { snprintf(buf, sizeof buf, " %zu", gm.tree_off[l]); tree += buf; }
    line(true, "  gm route=%s N=%d S=%d L=%d NC=%d SP=%d MV=%d ldW=%d plan_scale=%.17g init_once=%d dpp_chain=%d dpp_packed=%d sq_chain=%d dpp_cw=%d dpp_mode=%d gen_elems=%zu "
         "asm_split=%d asm_tail_wgs=%d windows=%s wideW=%d tree_off=%s aux=%d chain_s=%d events=%d,%d,%d", ROUTE_NAME(gm), gm.N, gm.S, gm.L, gm.NC, gm.SP, gm.MV, gm.ldW,
         gm.plan_scale, gm.init_once, gm.dpp_chain, gm.dpp_packed, gm.sq_chain, gm.dpp_cw, gm.dpp_mode(), gm.gen_elems(), gm.asm_split, gm.asm_tail_wgs, win.c_str(), gm.wideW,
         tree.c_str(), number(gm.aux), number(gm.chain_s), number(gm.ev_ready), number(gm.ev_fwd), number(gm.ev_p1));
    const void* ptrs[] = {gm.HsP, gm.HsPT, gm.A, gm.P, gm.K, gm.A2, gm.tree, gm.Y0, gm.Y1, gm.interP, gm.LamP, gm.SrcP, gm.KT, gm.PcT, gm.root, gm.zthin, gm.Psibnd, gm.Ebnd,
                          gm.Aoff, gm.partial, gm.HsSQ, gm.sqc, gm.wideP, gm.wideL, gm.wideC, gm.ts_Rall, gm.ts_Rtmp, gm.ts_Yr, gm.ts_Er};
    std::string s;
    for (const void* p : ptrs) s += " " + pointer(p);
    line(true, "  gm pointers%s", s.c_str());
}

// -1: not a problem of the GEMM path, else 0
static int run(const Problem& q) {
    const size_t nn = (size_t)q.n * q.n, nm = (size_t)q.n * q.m;
    std::vector<cplx> Hs((size_t)(q.k + 1) * nn);
    for (size_t i = 0; i < Hs.size(); ++i) { Hs[i].x = 0.001 * (double)(i % 97); Hs[i].y = -0.002 * (double)(i % 89); }
    if (q.antiherm)
        for (int i = 0; i <= q.k; ++i)
            for (int a = 0; a < q.n; ++a)
                for (int c = 0; c <= a; ++c) {
                    cplx& lo = Hs[((size_t)i * q.n + a) * q.n + c];
                    cplx& up = Hs[((size_t)i * q.n + c) * q.n + a];
                    if (a == c) lo.x = 0.0;
                    up.x = -lo.x; up.y = lo.y;
                }
    const bool antiherm = qoc_all_antihermitian(Hs.data(), q.n, q.k + 1);
    QocDev d;
    memset(&d, 0, sizeof d);
    d.n = q.n; d.k = q.k; d.steps = q.steps; d.m = q.m; d.state_transfer = q.st;
    d.T = q.T; d.s = q.st ? 0 : q.s;
    d.B = q.B; d.Bplan = q.Bplan; d.dt = 0.1;
    d.n_forb = q.reg == 1 ? 2 : 0;
    d.has_speed = q.reg == 2;
    if (!qoc_gemm_supported(d, antiherm)) return -1;
    // the trajectory view of an engine: every array a kernel of this path is handed is a traced allocation
    std::vector<void*> owned;
    const size_t B = (size_t)d.B, pts = B * (d.steps + 1), ks = B * d.k * d.steps;
    d.Hs = dev<cplx>(owned, Hs.size()); d.U0 = dev<cplx>(owned, nn); d.V = dev<cplx>(owned, nm); d.W = dev<cplx>(owned, nm); d.Psi0 = dev<cplx>(owned, nm);
    d.maxA = dev<double>(owned, d.k);
    if (d.n_forb > 0) { d.forb_state = dev<int>(owned, d.n_forb); d.forb_a = dev<double>(owned, d.n_forb); d.Fpop = dev<double>(owned, pts * d.n_forb * d.m); }
    d.base = dev<double>(owned, ks); d.w = dev<double>(owned, ks); d.u = dev<double>(owned, ks); d.dLdu = dev<double>(owned, ks); d.grad = dev<double>(owned, ks);
    d.inter = dev<cplx>(owned, pts * nm); d.Xfinal = dev<cplx>(owned, B * nn); d.ztau = dev<cplx>(owned, pts); d.zfin = dev<cplx>(owned, B);
    d.su_resid = dev<double>(owned, B); d.loss = dev<double>(owned, B); d.uscale = dev<double>(owned, B);

    if (q.sw || q.sw2) setenv("QOC_EXPERIMENTAL", "1", 1);
    if (q.sw) setenv(q.sw, q.sw_value, 1);
    if (q.sw2) setenv(q.sw2, q.sw2_value, 1);
    QocGemm gm;
    if (q.G > 0) { gm.ts_G = q.G; gm.ts_rank = -1; }
    gm.antiherm = antiherm;
    gm.direct_variant = q.variant;
    std::string msg;
    const int rc = qoc_gemm_setup(gm, d, Hs.data(), q.direct != 0, owned, msg);
    if (q.sw) unsetenv(q.sw);
    if (q.sw2) unsetenv(q.sw2);
    unsetenv("QOC_EXPERIMENTAL");
    line(true, "  setup rc=%d %s", rc, msg.c_str());
    if (rc == 0) {
        gm_digest(gm);
        line(true, "  lds_opt_in=%d", (int)qoc_gemm_lds_opt_in());
        line(true, "  lazy_final=%d zfree_backward=%d chunk_products=%s", (int)qoc_gemm_lazy_final(gm, d), (int)qoc_gemm_zfree_backward(gm, d),
             pointer(qoc_gemm_chunk_products(gm)).c_str());
        bool sharded = false;
        if (q.G > 0) {
            std::string why;
            sharded = qoc_gemm_ts_supported(gm, d, q.G, why);
            line(true, "  ts_supported=%d %s", (int)sharded, why.c_str());
            if (sharded) qoc_gemm_ts_ranges(gm, q.G);
        }
        for (int it = 0; it < 2; ++it) {                        // (gm.scan and init_once carry state from one iteration to the next)
            if (sharded) {
                line(true, " ts_evaluate");
                const int e = qoc_gemm_ts_evaluate(gm, d, nullptr, [&]() { line(true, " loss"); }, [&]() { line(true, " prof_begin"); return 0; },
                                                   [&]() { line(true, " prof_end"); return 0; });
                line(true, "  ts_evaluate rc=%d gather_inter rc=%d", e, qoc_gemm_ts_gather_inter(gm, d, nullptr));
                continue;
            }
            line(true, " expm"); qoc_gemm_expm(gm, d, nullptr);
            line(true, " forward"); qoc_gemm_forward(gm, d, nullptr);
            line(true, " backward"); BACKWARD(gm, d, nullptr, false);
            line(true, " backward, the tail sums the partials"); BACKWARD(gm, d, nullptr, true);
        }
        if (qoc_gemm_lazy_final(gm, d)) { line(true, " forward with_final"); qoc_gemm_forward(gm, d, nullptr, true); }
        gm_digest(gm);
    }
    line(true, " teardown"); qoc_gemm_teardown(gm);
    for (void* o : owned) free(o);
    g_allocs.clear();
    g_streams = g_events = 0;
    return 0;
}

int main(int argc, char** argv) {
    long every = 0, only = -1;
    const char* file = nullptr;
    for (int i = 1; i + 1 < argc; i += 2) {
        if (!strcmp(argv[i], "-v")) every = atol(argv[i + 1]);
        if (!strcmp(argv[i], "-o")) only = atol(argv[i + 1]);
        if (!strcmp(argv[i], "-f")) file = argv[i + 1];
    }
    for (const char* sw : SWITCHES) unsetenv(sw);
    unsetenv("QOC_EXPERIMENTAL");
    std::vector<Problem> table;
    //                       n   k  m  T  s st reg var dir ah  B Bplan steps G
    auto add = [&](Problem q) { if (q.Bplan == 0) q.Bplan = q.B; table.push_back(q); };
    const int regs[] = {0, 1, 2};
    // ---- direct route, butterfly chain: N = 32 and 64, every count of vector slots; 36 and 96 (seed, slice) items (k_gemm_assemble / _rows); k > 8
    for (int n : {24, 64}) for (int m : {1, 2, 3, 8}) for (int reg : regs) for (int B : {3, 8}) {
        Problem q{n, 2, m, 6, 0, 1, reg, 0, 1, 0, B, 0, 12, 0, nullptr, nullptr, nullptr, nullptr};
        if (n == 64 && m == 1) { q.sw = "QOC_CHAIN_DPP"; q.sw_value = "0"; }
        add(q);
    }
    add({24, 9, 1, 4, 0, 1, 1, 0, 1, 1, 8, 0, 12, 0});
    add({64, 9, 1, 4, 0, 1, 1, 0, 1, 1, 8, 0, 12, 0});
    for (int T : {1, 2}) for (int steps : {1, 2}) add({24, 2, 1, T, 0, 1, 0, 0, 1, 0, 2, 0, steps, 0});
    // ---- direct route, DPP chain: full, 10 / 12 / 14 active columns, packed (anti-Hermitian; more than 128 planned sets or n > 56), squared generators
    for (int reg : regs) for (int B : {3, 8}) {
        for (int n : {40, 48, 56, 64}) for (int ah = 0; ah < 2; ++ah) {
            add({n, 3, 1, 7, 0, 1, reg, 0, 1, ah, B, 0, 12, 0});
            add({n, 3, 1, 7, 0, 1, reg, 0, 1, ah, B, 200, 12, 0});
            add({n, 3, 1, 7, 0, 1, reg, 1, 1, ah, B, 0, 12, 0});
        }
        add({48, 3, 1, 7, 0, 1, reg, 0, 1, 1, B, 0, 12, 0, "QOC_DPP_ACTIVE_COLUMNS", "0"});
        for (int k = 1; k <= 8; ++k) add({k % 2 ? 64 : 44, k, 1, 3 + k, 0, 1, reg, 2, 1, 1, B, 0, 12, 0});
        add({64, 2, 1, 2, 0, 1, reg, 2, 1, 1, B, 0, 12, 0});             // (too few terms for the squared-generator chain)
        add({64, 2, 1, 15, 0, 1, reg, 2, 1, 1, B, 0, 12, 0});            // (too many)
    }
    // ---- the overlap windows: sources, steps >= 64, at most 128 sets -- with and without the CU mask, 2 and 4 windows, the switches that take it away
    for (int reg : {1, 2}) for (int var : {0, 2}) for (int n : {48, 64}) for (int ah = 0; ah < 2; ++ah) {
        for (int steps : {64, 100}) {
            add({n, 3, 1, 7, 0, 1, reg, var, 1, ah, 4, 0, steps, 0});
            add({n, 3, 1, 7, 0, 1, reg, var, 1, ah, 100, 0, steps, 0});                                       // (B + 16 > 112: no mask)
            add({n, 3, 1, 7, 0, 1, reg, var, 1, ah, 4, 0, steps, 0, "QOC_ASM_CUMASK", "0"});
            add({n, 3, 1, 7, 0, 1, reg, var, 1, ah, 4, 0, steps, 0, "QOC_ASM_CUMASK", "64"});
            add({n, 3, 1, 7, 0, 1, reg, var, 1, ah, 4, 0, steps, 0, "QOC_ASM_WINDOWS", "4"});
            add({n, 3, 1, 7, 0, 1, reg, var, 1, ah, 4, 0, steps, 0, "QOC_ASM_WINDOWS", "4", "QOC_ASM_CUMASK", "0"});
            add({n, 3, 1, 7, 0, 1, reg, var, 1, ah, 4, 0, steps, 0, "QOC_ASM_WINDOWS", "3", "QOC_ASM_SPLIT16", "15"});
            add({n, 3, 1, 7, 0, 1, reg, var, 1, ah, 4, 0, steps, 0, "QOC_ASM_TAIL_WGS", "1024", "QOC_ASM_SPLIT16", "0"});
            add({n, 3, 1, 7, 0, 1, reg, var, 1, ah, 4, 0, steps, 0, "QOC_ASM_OVERLAP", "0"});
            add({n, 3, 1, 7, 0, 1, reg, var, 1, ah, 4, 0, steps, 0, "QOC_CHAIN_DPP", "0"});
        }
        add({n, 3, 1, 7, 0, 1, reg, var, 1, ah, 129, 0, 64, 0});                                              // (more than 128 sets: no overlap)
        add({n, 3, 1, 7, 0, 1, reg, var, 1, ah, 4, 0, 63, 0});                                                // (too few steps)
    }
    add({64, 3, 1, 7, 0, 1, 0, 0, 1, 1, 4, 0, 64, 0});                                                        // (no sources: both chains side by side)
    // ---- persistent chains, state transfer that is not direct (anti-Hermitian generators)
    for (int n : {24, 64}) for (int m : {1, 2, 4, 8}) for (int reg : regs) for (int steps : {1, 3, 16, 21})
        add({n, 2, m, 5, 0, 1, reg, 0, 0, 1, m == 2 ? 1 : 3, 0, steps, 0});
    add({24, 2, 1, 5, 0, 1, 0, 0, 1, 1, 3, 0, 16, 1});                                                        // (time shards asked of a route without them)
    // ---- persistent chains, unitary: N = 32 and 64, one chunk and several, odd chunk counts, the planned batch moving the split-K factors
    for (int n : {32, 33}) for (int m : {1, 3, 8}) for (int reg : regs) for (int steps : {1, 3, 16, 20, 100}) for (int B : {1, 3})
        add({n, 2, m, 4, 2, 0, reg, 0, 0, 0, B, 0, steps, 0});
    for (int n : {32, 64}) for (int scale : {8, 16, 32, 64, 256, 1024}) for (int reg : {0, 1}) add({n, 2, 8, 4, 2, 0, reg, 0, 0, 0, 1, scale, 64, 0});
    add({32, 2, 1, 4, 2, 0, 0, 0, 0, 0, 1, 1, 5000, 1});
    // ---- launch per product: N = 96 and 128, m > 8 at N <= 64, wide gradient or not, one set and several, padded slices or not, Taylor degrees, scaling
    for (int n : {20, 40, 96, 128}) for (int m : {8, 9}) for (int st = 0; st < 2; ++st) for (int reg : regs) for (int B : {1, 3}) for (int steps : {1, 18, 20}) {
        if (n <= 64 && m <= 8) continue;                                                                      // (persistent)
        add({n, 2, m, st ? 6 : 5, st ? 0 : 3, st, reg, 0, 0, 1, B, 0, steps, 0});
    }
    for (int n : {40, 96, 128}) for (int T : {1, 2, 3, 4, 5, 6, 7, 30}) for (int s : {0, 3}) for (int st = 0; st < 2; ++st)
        add({n, 3, n == 40 ? 12 : 4, T, s, st, 0, 0, 0, 1, 2, 0, 18, 0});
    // (the planned batch moves the split-K factor and the kernel family: k_zgemm32 with 1 / 2 / 4 / 8 waves per tile, k_zgemm_wg with and without the
    // top block formed in flight)
    for (int n : {40, 64, 96, 128}) for (int scale : {1, 4, 16, 32, 64, 128, 256, 512, 2048}) for (int T : {4, 5}) for (int reg : {0, 1})
        add({n, 2, n <= 64 ? 9 : 4, T, 1, 0, reg, 0, 0, 0, 1, scale, 16, 0});
    add({256, 2, 4, 5, 1, 0, 0, 0, 0, 0, 1, 64, 16, 0});
    // ---- time shards: G = 1, 2 and the chunk count (steps = 20: 5 chunks of 4 slices), and what an engine refuses
    for (int G : {1, 2, 5, 6}) for (int steps : {18, 20}) for (int scale : {1, 64}) for (int T : {4, 5}) add({128, 2, 4, T, 1, 0, 0, 0, 0, 0, 1, scale, steps, G});
    add({128, 2, 4, 5, 1, 0, 1, 0, 0, 0, 1, 0, 20, 2});
    add({128, 2, 4, 5, 1, 0, 0, 0, 0, 0, 2, 0, 20, 2});
    add({96, 2, 4, 5, 1, 0, 0, 0, 0, 0, 1, 0, 20, 2});
    if (file) {             // the problems of a file instead: n k m T s state_transfer reg variant direct antiherm B Bplan steps G per line
        table.clear();
        FILE* f = fopen(file, "r");
        Problem q{};
        while (f && fscanf(f, "%d %d %d %d %d %d %d %d %d %d %d %d %d %d", &q.n, &q.k, &q.m, &q.T, &q.s, &q.st, &q.reg, &q.variant, &q.direct, &q.antiherm, &q.B, &q.Bplan, &q.steps,
                           &q.G) == 14) add(q);
        if (f) fclose(f);
        every = every > 0 ? every : 1;
    }
    long problems = 0, skipped = 0, total_lines = 0;
    unsigned long long combined = 1469598103934665603ull;
    for (size_t i = 0; i < table.size(); ++i) {
        if (only >= 0 && (long)i != only) continue;
        const Problem& q = table[i];
        g_verbose = only >= 0 || (every > 0 && i % every == 0);
        g_hash = 1469598103934665603ull; g_lines = 0; g_text.clear();
        if (run(q) != 0) { ++skipped; continue; }
        ++problems; total_lines += g_lines;
        combined = (combined ^ g_hash) * 1099511628211ull;
        printf("problem %zu n=%d k=%d m=%d T=%d s=%d state_transfer=%d reg=%d variant=%d direct=%d antiherm=%d B=%d Bplan=%d steps=%d G=%d %s=%s %s=%s lines=%ld hash=%016llx\n", i,
               q.n, q.k, q.m, q.T, q.s, q.st, q.reg, q.variant, q.direct, q.antiherm, q.B, q.Bplan, q.steps, q.G, q.sw ? q.sw : "switches", q.sw ? q.sw_value : "none",
               q.sw2 ? q.sw2 : "and", q.sw2 ? q.sw2_value : "none", g_lines, g_hash);
        if (g_verbose) fputs(g_text.c_str(), stdout);
    }
    printf("problems=%ld (of %zu: %ld are none of the GEMM path) trace_lines=%ld combined_hash=%016llx kernel_symbols=%zu\n", problems, table.size(), skipped, total_lines, combined,
           g_kernels.size());
    for (const std::string& k : g_kernels) printf("kernel %s\n", k.c_str());
    return 0;
}
