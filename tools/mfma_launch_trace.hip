// mfma_launch_trace.hip -- the launches of the MFMA path, traced on the host: for a table of problems, qoc_mfma_setup, every launcher (with and
// without a fused tail, the pulse regularisers both ways) and every read-back entry point an engine of that problem can call, through the shim
// launch_trace.h.  A dispatch edit is checked by building this program against csrc/ before and after it and comparing the two outputs:
//
//   hipcc --offload-arch=gfx950 -O1 -std=c++17 -Wno-unused-value -rdynamic -include tools/launch_trace.h -I <csrc> -I include \
//       tools/mfma_launch_trace.hip <csrc>/qoc_mfma_{expm,expm_inplace,forward,backward,latency}.hip -o mfma_launch_trace -ldl
//   ./mfma_launch_trace > after.txt          one line per problem: its parameters, the number of trace lines, a hash of them
//   ./mfma_launch_trace -v 1000 > after_v.txt     the trace lines themselves for every 1000th problem (-v 1: all of them), -o <i>: of problem i alone
//   ./mfma_launch_trace -f rows.txt          the problems of a file (twelve integers per line, see main) instead of the table, e.g. the rows of a test
//   ./mfma_launch_trace -s 0 -v 100000       the table without its experimental-switch problems (the kernels a production engine can reach)
//
// A trace line is a launch (kernel symbol from dladdr, grid, block, dynamic LDS, the integer arguments, the pointer arguments by allocation and
// offset, the per-call fields of the structs) or -- not hashed, -v only -- an LDS reservation.  The last lines count the kernels reached and the
// launches whose dynamic LDS qoc_mfma_setup had not reserved.  Needs no GPU; not part of build().
#include <dlfcn.h>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>
#include "qoc_kernels_mfma.h"

#if __has_include("qoc_mfma_plan.h")
#define PLAN plan,
#else
#define PLAN
#endif

struct Alloc { char* p; size_t bytes; };
static std::vector<Alloc> g_allocs;                    // of the current problem, in allocation order
static std::map<const void*, int> g_reserved;          // kernel -> bytes reserved, current problem
static std::set<std::string> g_kernels;
static std::string g_text;                             // the current problem's trace
static unsigned long long g_hash;
static long g_lines, g_unreserved;
static bool g_in_setup, g_verbose;
static const QocMfma* g_mf;

static void line(bool hashed, const char* fmt, ...) {
    char buf[1024];
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
static std::string pointer(const void* p) {
    if (!p) return "null";
    for (size_t a = 0; a < g_allocs.size(); ++a)
        if ((const char*)p >= g_allocs[a].p && (const char*)p < g_allocs[a].p + g_allocs[a].bytes) {
            char buf[64];
            snprintf(buf, sizeof buf, "a%zu+%zu", a, (size_t)((const char*)p - g_allocs[a].p));
            return buf;
        }
    return "stray";
}
hipError_t qoc_trace_malloc(void** p, size_t bytes) {
    *p = calloc(1, bytes ? bytes : 1);
    if (!*p) return hipErrorOutOfMemory;
    g_allocs.push_back({(char*)*p, bytes});
    line(true, "  alloc a%zu %zu", g_allocs.size() - 1, bytes);
    return hipSuccess;
}
hipError_t qoc_trace_reserve(const void* kernel, int bytes) {
    line(false, "  reserve%s %s %d", g_in_setup ? "" : " (in a launcher)", symbol(kernel).c_str(), bytes);
    if (g_in_setup && g_reserved[kernel] < bytes) g_reserved[kernel] = bytes;
    return hipSuccess;
}
hipError_t qoc_trace_launch(const void* kernel, dim3 grid, dim3 block, size_t lds, hipStream_t, const QocTraceArg* args, int count) {
    const std::string name = symbol(kernel);
    g_kernels.insert(name);
    std::string a;
    char buf[256];
    for (int i = 0; i < count; ++i) {
        const QocTraceArg& x = args[i];
        if (x.kind == QocTraceArg::INT) snprintf(buf, sizeof buf, " %lld", x.i);
        else if (x.kind == QocTraceArg::PTR) snprintf(buf, sizeof buf, " %s", pointer(x.p).c_str());
        else if (x.size == sizeof(QocDev)) {
            const QocDev& d = *(const QocDev*)x.p;
            snprintf(buf, sizeof buf, " d(skip_done=%d uscale_in_loss=%d u2=%s regs=%d%d%d%d)", d.skip_done, d.uscale_in_loss, pointer(d.u2).c_str(), d.has_amp, d.has_env,
                     d.has_dwdt, d.has_d2wdt2);
        }
        else if (x.size == sizeof(QocMfma)) snprintf(buf, sizeof buf, " mf%s", memcmp(x.p, g_mf, sizeof(QocMfma)) == 0 ? "" : "(ALTERED)");
        else if (x.size == sizeof(QocAdamDev)) { const QocAdamDev& ap = *(const QocAdamDev*)x.p; snprintf(buf, sizeof buf, " adam(mode=%d rate=%g max=%d)", ap.mode, ap.rate, ap.max_iterations); }
        else snprintf(buf, sizeof buf, " struct(%zu)", x.size);
        a += buf;
    }
    const bool reserved = lds == 0 || (g_reserved.count(kernel) && (size_t)g_reserved[kernel] >= lds);
    if (!reserved) ++g_unreserved;
    line(true, "  launch %s grid=%u,%u,%u block=%u,%u,%u lds=%zu%s", name.c_str(), grid.x, grid.y, grid.z, block.x, block.y, block.z, lds, a.c_str());
    if (!reserved) line(false, "    (dynamic LDS not reserved by qoc_mfma_setup)");
    return hipSuccess;
}

struct Problem { int n, k, m, degree, s, st, reg, variant, chunks, B, Bplan, steps; const char* sw; int sw_value; };
static const char* const SWITCHES[] = {"QOC_UPDOWN", "QOC_GRAD_RT", "QOC_ROWS_QA_FULL", "QOC_LAT_QA8", "QOC_LAT_OFFSETS_IN_SWEEP", "QOC_EXPM_HERM"};

static void mf_digest(const QocMfma& mf) {
    line(true, "  mf C=%d L=%d mq=%d NT=%d FR=%d G=%d NG=%d variant=%d store_T=%d updown=%d grad_rt=%d h_in_lds=%d latency=%d lat_sources=%d lat_src_fast=%d lat_dressed=%d "
         "exp=%d%d%d skew=%d,%d lds=%zu,%zu,%zu,%zu psigma=%.17g", mf.C, mf.L, mf.mq, mf.NT, mf.FR, mf.G, mf.NG, mf.variant, mf.store_T, mf.updown, mf.grad_rt, mf.h_in_lds,
         mf.latency, mf.lat_sources, mf.lat_src_fast, mf.lat_dressed, mf.exp_rows_qa_full, mf.exp_lat_qa8, mf.exp_lat_offsets_own, mf.skew_c, mf.skew_b, mf.du_lds,
         mf.grad_lds, mf.bwd_lds, mf.bwd_lds3, mf.psigma);
    const void* ptrs[] = {mf.HsD, mf.HfD, mf.HfT, mf.U0fD, mf.KfD, mf.KfT, mf.PfD, mf.PfT, mf.BndF, mf.BndA, mf.Aoff, mf.Goff, mf.LamD, mf.gpart, mf.GfD, mf.TfD, mf.PsiL,
                          mf.LamL, mf.LamS, mf.AoffL, mf.GoffL, mf.loss_part, mf.lat_count, mf.GfT};
    std::string s;
    for (const void* p : ptrs) s += " " + pointer(p);
    line(true, "  mf pointers%s", s.c_str());
}

// -1: not a problem of the MFMA path, else 0
static int run(const Problem& q, const std::vector<cplx>& Hs_table) {
    // the problems of the QOC_EXPM_HERM switch get exactly anti-Hermitian images (the table's are not: its other problems never pass the guard of the
    // symmetric exponential products, qoc_all_antihermitian), so that both values of the plan's expm_hermitian axis are traced
    std::vector<cplx> Hs(Hs_table);
    if (q.sw && !strcmp(q.sw, "QOC_EXPM_HERM"))
        for (int i = 0; i <= q.k; ++i)
            for (int a = 0; a < q.n; ++a)
                for (int c = 0; c <= a; ++c) {
                    cplx& lo = Hs[((size_t)i * q.n + a) * q.n + c];
                    cplx& up = Hs[((size_t)i * q.n + c) * q.n + a];
                    if (a == c) lo.x = 0.0;
                    up.x = -lo.x; up.y = lo.y;
                }
    QocDev d{};
    d.n = q.n; d.k = q.k; d.steps = q.steps; d.m = q.m; d.state_transfer = q.st;
    d.T = q.st ? q.degree + 1 : q.degree;                       // (the caller's taylor_terms)
    d.s = q.st ? 0 : q.s;
    d.B = q.B; d.Bplan = q.Bplan; d.dt = 0.1;
    // state regularisers: none, undressed forbidden levels, speed_up, 3 and 5 dressed levels
    d.n_forb = q.reg == 1 ? 2 : q.reg == 3 ? 3 : q.reg == 4 ? 5 : 0;
    d.forbid_dressed = q.reg >= 3;
    d.has_speed = q.reg == 2;
    if (!qoc_mfma_supported(d) || (q.variant == 5 && !qoc_mfma_latency_ok(d))) return -1;
    d.T = qoc_mfma_degree(d);                                   // as qoc_create does
    if (q.sw) { setenv("QOC_EXPERIMENTAL", "1", 1); setenv(q.sw, q.sw_value ? "1" : "0", 1); }
    std::vector<void*> owned;
    void* p = nullptr;
    (void)hipMalloc(&p, (size_t)d.n * d.n * sizeof(cplx)); owned.push_back(p); d.U0 = (const cplx*)p;
    (void)hipMalloc(&p, 64); owned.push_back(p); d.u2 = d.w2 = (double*)p;
    QocMfma mf;
    mf.variant = q.variant;
    std::string msg;
    g_mf = &mf;
    g_in_setup = true;
#if __has_include("qoc_mfma_plan.h")
    QocMfmaPlan plan;
    const int rc = qoc_mfma_setup(mf, plan, d, q.chunks, Hs.data(), owned, msg);
#else
    const int rc = qoc_mfma_setup(mf, d, q.chunks, Hs.data(), owned, msg);
#endif
    g_in_setup = false;
    if (q.sw) { unsetenv(q.sw); unsetenv("QOC_EXPERIMENTAL"); }
    line(true, "  setup rc=%d %s", rc, msg.c_str());
#if __has_include("qoc_mfma_plan.h")
    if (rc == 0 && plan.expm_variant == 8) line(true, "  expm_hermitian=%d", plan.expm_hermitian);
#endif
    if (rc == 0) {
        mf_digest(mf);
        const bool lat_own = mf.latency && (!mf.lat_sources || mf.lat_src_fast);
        QocAdamDev ap{};
        ap.mode = 1; ap.rate = 0.05; ap.max_iterations = 10;
        line(true, " expm"); qoc_mfma_launch_expm(PLAN mf, d, nullptr);
        for (int regs = 0; regs < 2; ++regs) {
            QocDev e = d;                                       // an iteration's copy, as the engine makes it
            e.has_amp = e.has_dwdt = regs; e.skip_done = regs; e.uscale_in_loss = regs;
            if (regs) { e.u2 = nullptr; e.w2 = nullptr; }
            line(true, " forward"); qoc_mfma_launch_forward(PLAN mf, e, nullptr);
            if (mf.latency) { line(true, " latency_sweeps"); qoc_mfma_latency_sweeps(PLAN mf, e, nullptr); }
            line(true, " backward"); qoc_mfma_launch_backward(PLAN mf, e, nullptr);
            if (lat_own) {
                line(true, " latency_gradient"); qoc_mfma_latency_gradient(PLAN mf, e, nullptr, nullptr);
                line(true, " latency_gradient fused"); qoc_mfma_latency_gradient(PLAN mf, e, &ap, nullptr);
            }
        }
        // the read-backs an engine of this problem makes (refresh_final, qoc_get_inter_vecs)
        if (mf.latency) { line(true, " final_state"); qoc_mfma_final_state(PLAN mf, d, nullptr); }
        if (mf.updown) { line(true, " final_state_batch"); qoc_mfma_final_state_batch(PLAN mf, d, nullptr); }
        line(true, " unpack_inter"); qoc_mfma_unpack_inter(PLAN mf, d, nullptr);
        if (d.state_transfer) { line(true, " uscale_state_transfer"); qoc_mfma_uscale_state_transfer(d, nullptr); }
    }
    for (void* o : owned) free(o);
    g_allocs.clear();
    g_reserved.clear();
    return 0;
}

int main(int argc, char** argv) {
    long every = 0, only = -1;
    const char* file = nullptr;
    bool switches = true;
    for (int i = 1; i + 1 < argc; i += 2) {
        if (!strcmp(argv[i], "-v")) every = atol(argv[i + 1]);
        if (!strcmp(argv[i], "-o")) only = atol(argv[i + 1]);
        if (!strcmp(argv[i], "-f")) file = argv[i + 1];
        if (!strcmp(argv[i], "-s")) switches = atoi(argv[i + 1]) != 0;
    }
    for (const char* sw : SWITCHES) unsetenv(sw);
    unsetenv("QOC_EXPERIMENTAL");
    // n: 1, 8, 9, 16 and both ends of every 4-wide strip from 17 to 64
    std::vector<int> ns = {1, 8, 9, 16};
    for (int a = 17; a <= 61; a += 4) { ns.push_back(a); ns.push_back(a + 3); }
    const int ms[] = {1, 8, 9, 16}, chunks[] = {0, 1, 4}, Bs[][2] = {{1, 1}, {3, 3}, {3, 64}, {64, 64}}, stepss[] = {8, 40};
    std::vector<cplx> Hs((size_t)9 * 64 * 64);
    for (size_t i = 0; i < Hs.size(); ++i) { Hs[i].x = 0.001 * (double)(i % 97); Hs[i].y = -0.002 * (double)(i % 89); }
    // Four sub-tables, each the full product of the dimensions whose conditions meet in the host code, the other dimensions drawn per problem
    // (a fixed generator: the same table in every build): shape x variant x state regulariser x mode; Taylor degree x scaling; batch x steps x chunks;
    // the experimental switches off and on
    std::vector<Problem> table;
    unsigned long long rng = 88172645463325252ull;
    auto draw = [&](int count) { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return (int)((rng >> 11) % (unsigned long long)count); };
    auto drawn = [&](Problem q, bool shape, bool taylor, bool batch) {
        if (!shape) { q.m = ms[draw(4)]; q.st = draw(2); }
        if (!taylor) { q.degree = 1 + draw(5); q.s = draw(2); }
        if (!batch) { const int b = draw(4); q.B = Bs[b][0]; q.Bplan = Bs[b][1]; q.steps = stepss[draw(2)]; q.chunks = chunks[draw(3)]; }
        table.push_back(q);
    };
    for (int n : ns) for (int k = 1; k <= 8; ++k) for (int v = 0; v <= 8; ++v) for (int reg = 0; reg < 5; ++reg) {
        Problem q{n, k, 0, 0, 0, 0, reg, v, 0, 0, 0, 0, nullptr, 0};
        for (int m : ms) for (int st = 0; st < 2; ++st) { q.m = m; q.st = st; drawn(q, true, false, false); }
        if (k % 3 == 1 || k == 5) for (int degree = 1; degree <= 5; ++degree) for (int s = 0; s < 2; ++s) { q.degree = degree; q.s = s; drawn(q, false, true, false); }
        if (k % 3 == 2 || k == 6) for (const auto& b : Bs) for (int steps : stepss) for (int c : chunks) { q.B = b[0]; q.Bplan = b[1]; q.steps = steps; q.chunks = c; drawn(q, false, false, true); }
        if (k % 2 == 1 && switches) for (const char* sw : SWITCHES) for (int on = 0; on < 2; ++on) { q.sw = sw; q.sw_value = on; drawn(q, false, false, false); }
    }
    if (file) {                                                 // the problems of a file instead: n k m degree s state_transfer reg variant chunks B Bplan steps per line
        table.clear();
        FILE* f = fopen(file, "r");
        Problem q{};
        while (f && fscanf(f, "%d %d %d %d %d %d %d %d %d %d %d %d", &q.n, &q.k, &q.m, &q.degree, &q.s, &q.st, &q.reg, &q.variant, &q.chunks, &q.B, &q.Bplan, &q.steps) == 12) table.push_back(q);
        if (f) fclose(f);
        every = every > 0 ? every : 1;
    }
    long problems = 0, skipped = 0, total_lines = 0;
    for (size_t i = 0; i < table.size(); ++i) {
        if (only >= 0 && (long)i != only) continue;
        const Problem& q = table[i];
        g_verbose = only >= 0 || (every > 0 && i % every == 0);
        g_hash = 1469598103934665603ull; g_lines = 0; g_text.clear();
        if (run(q, Hs) != 0) { ++skipped; continue; }
        ++problems; total_lines += g_lines;
        printf("problem %zu n=%d k=%d m=%d degree=%d s=%d state_transfer=%d reg=%d variant=%d chunks=%d B=%d Bplan=%d steps=%d %s=%d lines=%ld hash=%016llx\n", i, q.n, q.k, q.m,
               q.degree, q.s, q.st, q.reg, q.variant, q.chunks, q.B, q.Bplan, q.steps, q.sw ? q.sw : "switches", q.sw ? q.sw_value : 0, g_lines, g_hash);
        if (g_verbose) fputs(g_text.c_str(), stdout);
    }
    printf("problems=%ld (of %zu: %ld are none of the MFMA path) trace_lines=%ld kernel_symbols=%zu launches_with_unreserved_lds=%ld\n", problems, table.size(), skipped, total_lines,
           g_kernels.size(), g_unreserved);
    if (every > 0 || only >= 0) for (const std::string& k : g_kernels) printf("kernel %s\n", k.c_str());
    return 0;
}
