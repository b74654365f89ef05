// C ABI of libldpc_mi355x.so (declared in include/ldpc_mi355x.h): the entry points and their
// argument validation.  Graph preparation is graph_host.cpp, the device graph and the drop-in
// cache graph_device.cpp, the workspaces workspace.hpp.  Each synchronous host-pointer form
// stages into its workspace and shares the launches with its device-pointer (_dev) twin.  There
// is no CPU compute path: without a visible HIP device every entry point fails with LDPC_ENODEV.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "encode_host.hpp"
#include "graph_device.hpp"
#include "rate_match_host.hpp"
#include "workspace.hpp"

namespace ldpc {
namespace {
thread_local std::string g_err;
std::mutex g_mu;  // the drop-in graph cache and the host-buffer entry points (taken before Workspace::mu)
DropInCache g_dropin;

// The layout environment, read here and nowhere else: LDPC_NO_LOC_LAYOUT=1 builds no local-edge
// layout (tests run the other kernels on the same graphs), LDPC_NO_LOC_CHAIN=1 no chained layout
// beside it (fixed-count sum-product decodes then run on the plain one), LDPC_NO_LOC_TQ=1 keeps the chained
// layout on bp_loc_chain_kernel's generic instantiation at every width (tests hold the width's own to it), LDPC_LOC_T sets its thread count
// (shape experiments); an explicit loc_T (ldpc_debug_loc_variant) goes over the environment's.
// LDPC_NO_QC_KERNEL=1 keeps a quasi-cyclic graph's block-row schedule but not its row table
// (qc_Z = 0): it decodes on the table kernels (tests and A/B runs hold bp_qc_q_kernel to them).
LayoutOptions layout_options(int loc_T = 0) {
    LayoutOptions opt;
    const char *noloc = getenv("LDPC_NO_LOC_LAYOUT");
    opt.loc_layout = !(noloc && noloc[0] == '1');
    const char *nochain = getenv("LDPC_NO_LOC_CHAIN");
    opt.loc_chain = !(nochain && nochain[0] == '1');
    const char *notq = getenv("LDPC_NO_LOC_TQ");
    opt.loc_tq = !(notq && notq[0] == '1');
    if (const char *t = getenv("LDPC_LOC_T")) opt.loc_T = atoi(t);
    if (loc_T) opt.loc_T = loc_T;
    const char *noqc = getenv("LDPC_NO_QC_KERNEL");
    opt.qc_kernel = !(noqc && noqc[0] == '1');
    return opt;
}
}  // namespace

void set_error(const std::string &msg) { g_err = msg; }
}  // namespace ldpc

using namespace ldpc;

// The graph of a host-pointer form that takes edge lists: destroyed however the call ends
using OwnedGraph = std::unique_ptr<ldpc_graph, void (*)(ldpc_graph *)>;

// Workspace pointers from DevBuf::get: a failed one has said why
#define LDPC_ALLOCATED(ptrs)           \
    do {                               \
        if (!(ptrs)) return LDPC_EHIP; \
    } while (0)

// The rows of the ldpc_debug_*_plan entries.  calls[i] = {B, iters, algo, early_stop, mc,
// want_post}, planned by `plan` with those six; out + 9 i = {path, threads, grid, LDS bytes, col4
// (lds_slots; bp_layer_q_plan's: wg_per_cu), persistent, slab bytes, counter offset (-1: none),
// scratch bytes}; names + 64 i: the kernel's display name.  no_plan: the error (LDPC_EUNSUP, after
// every row is filled) when a call has no kernel; nullptr: such a row is an answer like any other.
template <typename Plan>
static int write_plans(int count, const int32_t *calls, int64_t *out, char *names, int BpPlan::*col4,
                       const char *no_plan, Plan plan) {
    bool none = false;
    for (int i = 0; i < count; ++i) {
        const int32_t *c = calls + 6 * (size_t)i;
        LDPC_REQUIRE(c[0] >= 0 && c[1] >= 0, "bad plan arguments");
        const BpPlan p = plan(c[0], c[1], c[2], c[3] != 0, c[4] != 0, c[5] != 0);
        int64_t *o = out + 9 * (size_t)i;
        o[0] = (int64_t)p.path; o[1] = p.threads; o[2] = p.grid; o[3] = (int64_t)p.lds; o[4] = p.*col4;
        o[5] = p.persistent; o[6] = (int64_t)p.slab; o[7] = p.counter; o[8] = (int64_t)p.scratch;
        snprintf(names + 64 * (size_t)i, 64, "%s", p.name);
        none |= p.path == BpPath::None;
    }
    if (none && no_plan) {
        set_error(no_plan);
        return LDPC_EUNSUP;
    }
    return LDPC_OK;
}

static const char *const kNoSchedule =
    "graph has no layer schedule (needs consistent lists, check degrees 1..32, no check holding a variable twice)";

// The three plan entries of a fixed code: its host layouts, then write_plans' rows of `plan` (bp_plan,
// bp_layer_plan or bp_layer_q_plan).  need_schedule: LDPC_EUNSUP up front for a graph without one.
template <typename Plan>
static int graph_plans(const int32_t *check_ptr, const int32_t *check_var, const int32_t *var_ptr,
                       const int32_t *var_slot, int n, int m, int count, const int32_t *calls, int cus, int64_t *out,
                       char *names, Plan plan, bool need_schedule, int BpPlan::*col4, const char *no_plan = nullptr) {
    LDPC_REQUIRE(count >= 0 && (count == 0 || (calls && out && names)) && cus > 0, "bad plan arguments");
    HostGraph h;
    LDPC_TRY(host_graph_from_csr(check_ptr, check_var, var_ptr, var_slot, n, m, h));
    GraphShape g;
    HostLayouts L;
    host_layouts(h, g, L, true, layout_options());
    if (need_schedule && g.lay_L <= 0) {
        set_error(kNoSchedule);
        return LDPC_EUNSUP;
    }
    return write_plans(count, calls, out, names, col4, no_plan,
                       [&](int B, int iters, int algo, bool et, bool mc, bool want_post) {
                           return plan(g, B, iters, algo, et, mc, want_post, cus);
                       });
}

// ---- the soft decoders' path from an entry to a launch: a SoftCall and a family (ldpc_internal.hpp)
// The call of a decode (post nullptr: no posteriors asked for, early stop may take the hard-decision path)
static SoftCall decode_call(int B, int max_iters, int algo, float alpha, int early_stop, const float *llr, void *post,
                            uint8_t *hard, int32_t *its) {
    SoftCall c{B, max_iters, algo, alpha, early_stop != 0, false};
    c.llr = llr, c.post = post, c.hard = hard, c.its = its;
    // LDPC_NO_WIDE_IO=1, read per call: the fixed-count bp_loc_kernel decodes move their rows 4 bytes
    // and 1 byte at a time whatever the alignment (tests hold the 16-byte path to this one)
    const char *nowide = getenv("LDPC_NO_WIDE_IO");
    c.narrow_io = nowide && nowide[0] == '1';
    return c;
}
// The call of a fused Monte-Carlo batch (mc_entry gives it trial and its)
static SoftCall mc_call(int B, int max_iters, int algo, float alpha, int early_stop, const ChanArgs &ch,
                        uint64_t first_cw) {
    SoftCall c{B, max_iters, algo, alpha, early_stop != 0, true};
    c.ch = ch, c.first_cw = first_cw;
    return c;
}

// The one step every soft call goes through, its workspace locked: plan once, take the plan's
// scratch from the workspace -- the one place a buffer shorter than the plan's is refused -- and
// launch from that same plan.  B > 0.
template <typename Family>
static int soft_launch(Workspace &ws, const Family &f, const SoftCall &c, hipStream_t s) {
    const BpPlan p = f.plan(c, device_cus());
    float *scratch = p.scratch ? ws.scratch.get<float>((p.scratch + 3) / 4) : nullptr;
    LDPC_ALLOCATED(scratch || !p.scratch);
    if (p.scratch > (scratch ? ws.scratch.cap : 0)) LDPC_HIP(hipErrorInvalidValue);
    LDPC_HIP(f.launch(p, c, scratch, s));
    return LDPC_OK;
}

// The device decode entries' driver: g_mu, then the workspace's lock, both held across the
// (asynchronous) launch (workspace.hpp).  Arguments validated by the entry; B > 0.
template <typename Family>
static int decode_entry(const Family &f, const SoftCall &c, void *stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    Workspace &ws = workspace(stream);
    std::lock_guard<std::mutex> wl(ws.mu);
    return soft_launch(ws, f, c, static_cast<hipStream_t>(stream));
}

// The fused Monte-Carlo entries' driver: this (device, stream)'s workspace lock only, so devices
// launch in parallel; the per-trial curves [B][max_iters + 1] and iteration counts [B] that
// decode(ws, c, s) has the batch's kernels fill -- after sampling the trials' graphs, for an
// ensemble -- then the reducer with its cutoff.  Arguments validated by the entry; B > 0.
template <typename Decode>
static int mc_entry(SoftCall c, int expurgation, int64_t stop_frame_errors, int64_t *d_counters, void *stream,
                    Decode decode) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    Workspace &ws = workspace(stream);
    std::lock_guard<std::mutex> wl(ws.mu);
    c.trial = ws.trial.get<int32_t>((size_t)c.B * (c.max_iters + 1));
    c.its = ws.its.get<int32_t>(c.B);
    int32_t *cut = ws.cutoff.get<int32_t>(4);
    LDPC_ALLOCATED(c.trial && c.its && cut);
    LDPC_TRY(decode(ws, c, s));
    LDPC_HIP(launch_mc_reduce(c.trial, c.its, c.B, c.max_iters, expurgation, stop_frame_errors, d_counters, cut, s));
    return LDPC_OK;
}
// mc_entry's `decode` of a fixed code's family: soft_launch alone
template <typename Family>
static auto soft_decode(const Family &f) {
    return [f](Workspace &ws, const SoftCall &c, hipStream_t s) { return soft_launch(ws, f, c, s); };
}

extern "C" {

const char *ldpc_last_error(void) { return g_err.c_str(); }

int ldpc_device_count(void) {
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) return 0;
    return c;
}

int ldpc_set_device(int device) {
    LDPC_TRY(require_device());
    LDPC_HIP(hipSetDevice(device));
    return LDPC_OK;
}

int ldpc_sync(void *stream) {
    LDPC_TRY(require_device());
    LDPC_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return LDPC_OK;
}

int ldpc_graph_create(const int32_t *variable_to_check_list, const int32_t *check_to_variable_list, int n, int k,
                      int dv, int dc, ldpc_graph **out) {
    LDPC_REQUIRE(out, "null output handle");
    HostGraph h;
    LDPC_TRY(host_graph_from_lists(variable_to_check_list, check_to_variable_list, n, k, dv, dc, h));
    return device_graph(h, out, true, layout_options());
}

int ldpc_graph_create_csr(const int32_t *check_ptr, const int32_t *check_var, const int32_t *var_ptr,
                          const int32_t *var_slot, int n, int m, ldpc_graph **out) {
    LDPC_REQUIRE(out, "null output handle");
    HostGraph h;
    LDPC_TRY(host_graph_from_csr(check_ptr, check_var, var_ptr, var_slot, n, m, h));
    return device_graph(h, out, true, layout_options());
}

int ldpc_graph_create_qc(int mb, int nb, int Z, const int32_t *base, ldpc_graph **out) {
    LDPC_REQUIRE(out, "null output handle");
    HostGraph h;
    QcCode qc;
    LDPC_TRY(host_graph_from_qc(mb, nb, Z, base, h, qc));
    LayoutOptions opt = layout_options();
    opt.qc = &qc;
    return device_graph(h, out, true, opt);
}

const char *ldpc_graph_layer_rule(const ldpc_graph *g) { return g && g->lay_block_rows ? kQcLayerRule : kLayerRule; }

void ldpc_graph_destroy(ldpc_graph *g) { destroy_device_graph(g); }

int ldpc_graph_info(const ldpc_graph *g, int32_t *n, int32_t *m, int32_t *num_edges) {
    LDPC_REQUIRE(g, "null graph");
    if (n) *n = g->n;
    if (m) *m = g->m;
    if (num_edges) *num_edges = g->E;
    return LDPC_OK;
}

// --------------------------- host-only layout queries ----------------------
int ldpc_debug_lane_layout(const int32_t *variable_to_check_list, const int32_t *check_to_variable_list, int n,
                           int k, int dv, int dc, int32_t *T, int32_t *VPT, int32_t *lane_var, int32_t *lane_slot) {
    LDPC_REQUIRE(T && VPT, "null T / VPT");
    HostGraph h;
    LDPC_TRY(host_graph_from_lists(variable_to_check_list, check_to_variable_list, n, k, dv, dc, h));
    int t = 0, v = 0;
    LDPC_REQUIRE(h.consistent && lds_shape(n, t, v), "no LDS-resident layout for this graph");
    *T = t;
    *VPT = v;
    if (!lane_var || !lane_slot) return LDPC_OK;
    std::vector<int32_t> lv, ls;
    build_lane_layout(h, t, v, lv, ls);
    std::copy(lv.begin(), lv.end(), lane_var);
    std::copy(ls.begin(), ls.end(), lane_slot);
    return LDPC_OK;
}

int ldpc_debug_irr_layout(const int32_t *check_ptr, const int32_t *check_var, const int32_t *var_ptr,
                          const int32_t *var_slot, int n, int m, int32_t *shape, int32_t *lane, int32_t *cdeg) {
    LDPC_REQUIRE(shape, "null shape");
    HostGraph h;
    LDPC_TRY(host_graph_from_csr(check_ptr, check_var, var_ptr, var_slot, n, m, h));
    std::vector<int32_t> ln, cd;
    int VPT = 0, KC = 0, DC = 0, S = 0, P = 0;
    if (!h.consistent || !build_irr_layout(h, VPT, KC, DC, S, P, ln, cd)) {
        set_error("graph outside the irregular kernel's range");
        return LDPC_EUNSUP;
    }
    shape[0] = VPT; shape[1] = KC; shape[2] = DC; shape[3] = S; shape[4] = P;
    if (lane) std::copy(ln.begin(), ln.end(), lane);
    if (cdeg) std::copy(cd.begin(), cd.end(), cdeg);
    return LDPC_OK;
}

int ldpc_debug_loc_layout(const int32_t *check_ptr, const int32_t *check_var, const int32_t *var_ptr,
                          const int32_t *var_slot, int n, int m, int T, int32_t *shape, int32_t *var, int32_t *pos,
                          int32_t *info) {
    LDPC_REQUIRE(shape, "null shape");
    LDPC_REQUIRE(T == 256 || T == 512 || T == 1024, "T must be 256, 512 or 1024");
    HostGraph h;
    LDPC_TRY(host_graph_from_csr(check_ptr, check_var, var_ptr, var_slot, n, m, h));
    LocLayout L;
    L.T = T;
    if (!h.consistent || !build_loc_layout(h.n, h.m, h.cptr, h.cvar, h.vptr, h.vslot, L)) {
        set_error("graph has no local-edge layout (needs n = 2m, a perfect local matching, even degree classes)");
        return LDPC_EUNSUP;
    }
    shape[0] = L.T; shape[1] = L.KP; shape[2] = L.DVN; shape[3] = L.P; shape[4] = L.words;
    shape[5] = L.ncls; shape[6] = (int32_t)std::min<long>(L.conflicts, 0x7fffffff);
    for (int i = 0; i < kLocMaxCls; ++i) {
        shape[7 + i] = L.cls_q[i];
        shape[7 + kLocMaxCls + 1 + i] = L.cls_d[i];
        shape[7 + 2 * kLocMaxCls + 1 + i] = L.cls_w[i];
    }
    shape[7 + kLocMaxCls] = L.cls_q[kLocMaxCls];
    shape[7 + 3 * kLocMaxCls + 1] = L.cls_w[kLocMaxCls];
    shape[22] = L.DVN0 | (L.ABS0 ? 256 : 0);
    shape[23] = L.DVN1 | (L.ABS1 ? 256 : 0);
    if (var) std::copy(L.var.begin(), L.var.end(), var);
    if (pos) std::copy(L.pos.begin(), L.pos.end(), pos);
    if (info) std::copy(L.info.begin(), L.info.end(), info);
    return LDPC_OK;
}

// The chained layout (build_loc_chain_layout) of the plain T = 512 layout: shape = {Tq, KP, chain
// links per thread, words, conflicts, T}; var / pos / info as ldpc_debug_loc_layout's, chk
// [2 KP][T]: the check at pair slot k, half h of thread t (row 2k + h; -1: none).  LDPC_EUNSUP
// when the graph has no chained layout.
int ldpc_debug_loc_chain_layout(const int32_t *check_ptr, const int32_t *check_var, const int32_t *var_ptr,
                                const int32_t *var_slot, int n, int m, int32_t *shape, int32_t *var, int32_t *pos,
                                int32_t *info, int32_t *chk) {
    LDPC_REQUIRE(shape, "null shape");
    HostGraph h;
    LDPC_TRY(host_graph_from_csr(check_ptr, check_var, var_ptr, var_slot, n, m, h));
    LocLayout L;
    L.T = kLocChainT;
    LocChainLayout C;
    if (!h.consistent || !build_loc_layout(h.n, h.m, h.cptr, h.cvar, h.vptr, h.vslot, L) ||
        !build_loc_chain_layout(h.n, h.m, h.cptr, h.cvar, h.vptr, h.vslot, L, C)) {
        set_error("no chained layout (needs the (3,6) 512 x 5 local-edge shape, P a multiple of 5, no repeated variable "
                  "in a check, and a chain cover)");
        return LDPC_EUNSUP;
    }
    shape[0] = C.Tq; shape[1] = kLocChainKP; shape[2] = kLocChainCL; shape[3] = C.words;
    shape[4] = (int32_t)std::min<long>(C.conflicts, 0x7fffffff); shape[5] = kLocChainT;
    if (var) std::copy(C.var.begin(), C.var.end(), var);
    if (pos) std::copy(C.pos.begin(), C.pos.end(), pos);
    if (info) std::copy(C.info.begin(), C.info.end(), info);
    if (chk) std::copy(C.chk.begin(), C.chk.end(), chk);
    return LDPC_OK;
}

int ldpc_debug_loc_variant(const int32_t *check_ptr, const int32_t *check_var, const int32_t *var_ptr,
                           const int32_t *var_slot, int n, int m, int T, int32_t *variant) {
    LDPC_REQUIRE(variant, "null variant");
    LDPC_REQUIRE(T == 256 || T == 512 || T == 1024, "T must be 256, 512 or 1024");
    HostGraph h;
    LDPC_TRY(host_graph_from_csr(check_ptr, check_var, var_ptr, var_slot, n, m, h));
    *variant = kLocNone;
    if (!h.consistent) return LDPC_OK;
    GraphShape g;
    HostLayouts L;
    host_layouts(h, g, L, true, layout_options(T));  // the shipped layout rules, at the asked-for thread count
    *variant = loc_variant(g);
    return LDPC_OK;
}

// The launch plans (bp_plan) of `count` soft-decoding calls on one graph, from the host layouts
// alone; calls / out / names: write_plans'.
int ldpc_debug_bp_plan(const int32_t *check_ptr, const int32_t *check_var, const int32_t *var_ptr,
                       const int32_t *var_slot, int n, int m, int count, const int32_t *calls, int cus, int64_t *out,
                       char *names) {
    return graph_plans(check_ptr, check_var, var_ptr, var_slot, n, m, count, calls, cus, out, names, bp_plan, false,
                       &BpPlan::lds_slots);
}

// The same with the calls' row pointers (addresses only, nothing is read through them; FloodFamily::plan's
// steps): calls[i] = {B, iters, algo, early_stop, mc, llr, post, hard, narrow}, want_post = post != 0;
// out + 11 i = ldpc_debug_bp_plan's nine, then wide_io and the words of bp_loc_kernel's message LDS
// (0 on another path).
int ldpc_debug_bp_plan_io(const int32_t *check_ptr, const int32_t *check_var, const int32_t *var_ptr,
                          const int32_t *var_slot, int n, int m, int count, const int64_t *calls, int cus, int64_t *out,
                          char *names) {
    LDPC_REQUIRE(count >= 0 && (count == 0 || (calls && out && names)) && cus > 0, "bad plan arguments");
    HostGraph h;
    LDPC_TRY(host_graph_from_csr(check_ptr, check_var, var_ptr, var_slot, n, m, h));
    GraphShape g;
    HostLayouts L;
    host_layouts(h, g, L, true, layout_options());
    for (int i = 0; i < count; ++i) {
        const int64_t *c = calls + 9 * (size_t)i;
        LDPC_REQUIRE(c[0] >= 0 && c[1] >= 0, "bad plan arguments");
        const bool et = c[3] != 0, mc = c[4] != 0;
        BpPlan p = bp_plan(g, (int)c[0], (int)c[1], (int)c[2], et, mc, c[6] != 0, cus);
        p.wide_io = bp_wide_io(p, g, et, mc, reinterpret_cast<const void *>(c[5]), reinterpret_cast<const void *>(c[6]),
                               reinterpret_cast<const void *>(c[7]), c[8] != 0);
        int64_t *o = out + 11 * (size_t)i;
        o[0] = (int64_t)p.path; o[1] = p.threads; o[2] = p.grid; o[3] = (int64_t)p.lds; o[4] = p.lds_slots;
        o[5] = p.persistent; o[6] = (int64_t)p.slab; o[7] = p.counter; o[8] = (int64_t)p.scratch;
        o[9] = p.wide_io;
        o[10] = p.path == BpPath::Loc ? (int64_t)loc_msg_words(p.chain ? g.chn_words : g.loc_words, g.n) : 0;
        snprintf(names + 64 * (size_t)i, 64, "%s", p.name);
    }
    return LDPC_OK;
}

// The launch width (BpPlan::width: the threads a workgroup is launched with) of ldpc_debug_bp_plan's
// calls, one per call: the chained layout's Tq for the call that takes it, else the plan's threads.
int ldpc_debug_bp_plan_width(const int32_t *check_ptr, const int32_t *check_var, const int32_t *var_ptr,
                             const int32_t *var_slot, int n, int m, int count, const int32_t *calls, int cus,
                             int64_t *out) {
    LDPC_REQUIRE(count >= 0 && (count == 0 || (calls && out)) && cus > 0, "bad plan arguments");
    HostGraph h;
    LDPC_TRY(host_graph_from_csr(check_ptr, check_var, var_ptr, var_slot, n, m, h));
    GraphShape g;
    HostLayouts L;
    host_layouts(h, g, L, true, layout_options());
    for (int i = 0; i < count; ++i) {
        const int32_t *c = calls + 6 * (size_t)i;
        LDPC_REQUIRE(c[0] >= 0 && c[1] >= 0, "bad plan arguments");
        out[i] = bp_plan(g, c[0], c[1], c[2], c[3] != 0, c[4] != 0, c[5] != 0, cus).width;
    }
    return LDPC_OK;
}

// The compile-time width (BpPlan::tq) of the same calls, one per call: the chained call's Tq where
// LDPC_LOC_CHAIN_TQ lists it and LDPC_NO_LOC_TQ is not set, else 0 (the generic instantiation, every other kernel).
int ldpc_debug_bp_plan_tq(const int32_t *check_ptr, const int32_t *check_var, const int32_t *var_ptr,
                          const int32_t *var_slot, int n, int m, int count, const int32_t *calls, int cus,
                          int64_t *out) {
    LDPC_REQUIRE(count >= 0 && (count == 0 || (calls && out)) && cus > 0, "bad plan arguments");
    HostGraph h;
    LDPC_TRY(host_graph_from_csr(check_ptr, check_var, var_ptr, var_slot, n, m, h));
    GraphShape g;
    HostLayouts L;
    host_layouts(h, g, L, true, layout_options());
    for (int i = 0; i < count; ++i) {
        const int32_t *c = calls + 6 * (size_t)i;
        LDPC_REQUIRE(c[0] >= 0 && c[1] >= 0, "bad plan arguments");
        out[i] = bp_plan(g, c[0], c[1], c[2], c[3] != 0, c[4] != 0, c[5] != 0, cus).tq;
    }
    return LDPC_OK;
}

// ldpc_bp_decode_batch_dev's fixed-count sum-product decode from its own plan but for BpPlan::tq, which is `tq`:
// what the launcher answers to a plan whose compile-time width is not the graph's (LDPC_EHIP, nothing started).
int ldpc_debug_bp_decode_tq(const ldpc_graph *g, int tq, const float *d_llr, int B, int max_iters, float *d_post,
                            uint8_t *d_hard, int32_t *d_its, void *stream) {
    LDPC_REQUIRE(g && d_llr && B > 0 && max_iters >= 0 && tq >= 0, "bad soft batch arguments");
    LDPC_REQUIRE(g->consistent, "soft decoding needs consistent edge lists");
    const SoftCall c = decode_call(B, max_iters, LDPC_ALGO_SPA, 1.0f, 0, d_llr, d_post, d_hard, d_its);
    const FloodFamily f{*g};
    std::lock_guard<std::mutex> lk(g_mu);
    Workspace &ws = workspace(stream);
    std::lock_guard<std::mutex> wl(ws.mu);
    BpPlan p = f.plan(c, device_cus());
    LDPC_REQUIRE(p.path == BpPath::Loc && p.chain && p.scratch == 0, "not a chained-layout call");
    p.tq = tq;
    LDPC_HIP(f.launch(p, c, nullptr, static_cast<hipStream_t>(stream)));
    return LDPC_OK;
}

// The launch plans (bec_plan) of `count` BEC calls on an (n, m) graph of check degree dc (0:
// irregular), from the shape alone.  calls[i] = {mode, B, iters, peel_cap}; out + 9 i = {kernel,
// threads, W, plane bytes, codewords per workgroup, grid, LDS bytes, F, LDS cap}; names + 64 i:
// the kernel's display name.  A call that no kernel holds is a row of its own (BecKernel::None).
int ldpc_debug_bec_plan(int n, int m, int dc, int count, const int32_t *calls, int64_t *out, char *names) {
    LDPC_REQUIRE(n > 0 && m > 0 && dc >= 0 && count >= 0 && (count == 0 || (calls && out && names)),
                 "bad plan arguments");
    for (int i = 0; i < count; ++i) {
        const int32_t *c = calls + 4 * (size_t)i;
        LDPC_REQUIRE(c[0] >= 0 && c[0] <= 2 && c[1] >= 0 && c[2] >= 0, "bad plan arguments");
        const BecPlan p = bec_plan(n, m, dc, c[1], c[2], static_cast<BecMode>(c[0]), c[3]);
        int64_t *o = out + 9 * (size_t)i;
        o[0] = (int64_t)p.kernel; o[1] = p.threads; o[2] = p.W; o[3] = p.plane; o[4] = p.cw_per_wg;
        o[5] = p.grid; o[6] = (int64_t)p.lds; o[7] = p.F; o[8] = (int64_t)p.cap;
        snprintf(names + 64 * (size_t)i, 64, "%s", p.name);
    }
    return LDPC_OK;
}

// The launch plan (sample_plan) of one sampler call, from the shape alone; out / names: the header's.
int ldpc_debug_sample_plan(int n, int m, int E, int max_cdeg, int max_vdeg, int regular, int dv, int G, int cus,
                           int64_t *out, char *names) {
    LDPC_REQUIRE(n > 0 && m > 0 && E > 0 && max_cdeg > 0 && max_vdeg > 0 && G >= 0 && cus >= 0 && out && names &&
                     (!regular || dv > 0),
                 "bad plan arguments");
    const SamplePlan p = sample_plan(n, m, E, max_cdeg, max_vdeg, regular != 0, dv, G, cus);
    const int64_t row[16] = {p.seq, p.threads, p.K, (int64_t)p.lds, p.bw, p.ring, p.fb, p.fbu,
                             p.emit_fb, (int64_t)p.mdv, p.V, p.nch, p.row, (int64_t)p.vs_lds, p.per_cu, p.W};
    std::copy(row, row + 16, out);
    snprintf(names, 64, "%s", p.draw);
    snprintf(names + 64, 64, "%s", p.var_side);
    snprintf(names + 128, 64, "%s", p.search);
    return LDPC_OK;
}

const char *ldpc_bp_kernel_name(const ldpc_graph *g, int early_stop) {
    return g ? bp_kernel_name(*g, early_stop) : "none";
}

// --------------------------- BEC -------------------------------------------
// Arguments validated by the caller; B > 0.
static int bec_launch(const ldpc_graph *g, uint8_t *d_words, int B, int max_iters, int32_t *d_errors, int32_t *d_its,
                      hipStream_t s) {
    if (max_iters == 0) LDPC_HIP(hipMemsetAsync(d_its, 0, sizeof(int32_t) * B, s));
    else LDPC_HIP(launch_bec_decode(*g, d_words, B, max_iters, d_errors, d_its, s));
    return LDPC_OK;
}

int ldpc_bec_decode_batch_dev(const ldpc_graph *g, uint8_t *d_words, int B, int max_iters, int32_t *d_errors,
                              int32_t *d_its, void *stream) {
    LDPC_REQUIRE(g && (B == 0 || (d_words && d_errors && d_its)) && B >= 0 && max_iters >= 0, "bad BEC batch arguments");
    return B ? bec_launch(g, d_words, B, max_iters, d_errors, d_its, static_cast<hipStream_t>(stream)) : LDPC_OK;
}

int ldpc_bec_decode_batch(const int32_t *variable_to_check_list, const int32_t *check_to_variable_list, int n,
                          int k, int dv, int dc, uint8_t *words, int B, int max_iters, int32_t *errors,
                          int32_t *its) {
    LDPC_REQUIRE((B == 0 || (words && errors && its)) && B >= 0 && max_iters >= 0, "bad BEC batch arguments");
    ldpc_graph *g = nullptr;
    LDPC_TRY(ldpc_graph_create(variable_to_check_list, check_to_variable_list, n, k, dv, dc, &g));
    const OwnedGraph owner(g, ldpc_graph_destroy);
    if (B == 0) return LDPC_OK;
    const size_t nb = (size_t)B * n, eb = sizeof(int32_t) * (size_t)B * max_iters;
    for (size_t i = 0; i < nb; ++i) LDPC_REQUIRE(words[i] <= 2, "channel word value outside {0, 1, 2}");
    std::lock_guard<std::mutex> lk(g_mu);
    Workspace &ws = workspace(nullptr);
    std::lock_guard<std::mutex> wl(ws.mu);
    uint8_t *dw = ws.words.get<uint8_t>(nb);
    int32_t *de = ws.errors.get<int32_t>((size_t)B * std::max(max_iters, 1)), *di = ws.itsb.get<int32_t>(B);
    LDPC_ALLOCATED(dw && de && di);
    LDPC_HIP(hipMemcpy(dw, words, nb, hipMemcpyHostToDevice));
    if (eb) LDPC_HIP(hipMemcpy(de, errors, eb, hipMemcpyHostToDevice));
    LDPC_TRY(bec_launch(g, dw, B, max_iters, de, di, nullptr));
    LDPC_HIP(hipDeviceSynchronize());
    LDPC_HIP(hipMemcpy(words, dw, nb, hipMemcpyDeviceToHost));
    if (eb) LDPC_HIP(hipMemcpy(errors, de, eb, hipMemcpyDeviceToHost));
    LDPC_HIP(hipMemcpy(its, di, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost));
    return LDPC_OK;
}

// Drop-in for message_passing.c:7: validate, find the graph, stage, decode, copy back.
int message_passing(int *Mvc, int iterations, int *variable_to_check_list, int *check_to_variable_list,
                    int *errors, int n, int k, int dv, int dc) {
    if (iterations <= 0) return 0;  // the reference loop body never runs
    LDPC_REQUIRE(Mvc && errors && variable_to_check_list && check_to_variable_list, "null Mvc / errors / lists");
    LDPC_REQUIRE(n > 0 && dv > 0 && dc > 0 && k >= 0 && k < n, "bad (n, k, dv, dc)");
    LDPC_TRY(require_device());
    // One lock across the cache lookup and the decode: another thread replacing the cached
    // graph cannot free it while this call still uses it.
    std::lock_guard<std::mutex> lk(g_mu);
    DropInCache &c = g_dropin;
    int dev = 0;
    (void)hipGetDevice(&dev);
    LDPC_TRY(c.lookup_or_build(variable_to_check_list, check_to_variable_list, n, k, dv, dc, dev));
    const size_t wb = ((size_t)n + 15) & ~(size_t)15, eb = (size_t)4 * iterations;
    LDPC_TRY(c.staging(wb + eb + 16));
    uint8_t *pw = c.pin;
    for (int v = 0; v < n; ++v) {
        LDPC_REQUIRE(Mvc[v] >= 0 && Mvc[v] <= 2, "Mvc value outside {0, 1, 2}");
        pw[v] = (uint8_t)Mvc[v];
    }
    memcpy(c.pin + wb, errors, eb);  // the reference accumulates into the caller's errors[]
    LDPC_HIP(hipMemcpyAsync(c.dbuf, c.pin, wb + eb, hipMemcpyHostToDevice, c.s));
    LDPC_TRY(bec_launch(c.g, c.dbuf, 1, iterations, reinterpret_cast<int32_t *>(c.dbuf + wb),
                        reinterpret_cast<int32_t *>(c.dbuf + wb + eb), c.s));
    LDPC_HIP(hipMemcpyAsync(c.pin, c.dbuf, wb + eb + 4, hipMemcpyDeviceToHost, c.s));
    LDPC_HIP(hipStreamSynchronize(c.s));
    for (int v = 0; v < n; ++v) Mvc[v] = pw[v];
    memcpy(errors, c.pin + wb, eb);
    int32_t it = 0;
    memcpy(&it, c.pin + wb + eb, 4);
    return it;
}

// --------------------------- soft ------------------------------------------
int ldpc_bp_decode_batch_dev(const ldpc_graph *g, const float *d_llr, int B, int max_iters, int algo, float alpha,
                             int early_stop, float *d_post, uint8_t *d_hard, int32_t *d_its, void *stream) {
    LDPC_REQUIRE(g && (B == 0 || d_llr) && B >= 0 && max_iters >= 0, "bad soft batch arguments");
    LDPC_REQUIRE(algo == LDPC_ALGO_SPA || algo == LDPC_ALGO_MINSUM, "algo must be LDPC_ALGO_SPA or LDPC_ALGO_MINSUM");
    LDPC_REQUIRE(g->consistent,
                 "soft decoding needs consistent edge lists (each (v,c) pair listed equally often on both sides)");
    if (!strcmp(bp_kernel_name(*g, early_stop), "none")) {
        set_error("no soft kernel for this graph (check degree > 32)");
        return LDPC_EUNSUP;
    }
    if (B == 0) return LDPC_OK;
    const SoftCall c = decode_call(B, max_iters, algo, alpha, early_stop, d_llr, d_post, d_hard, d_its);
    return decode_entry(FloodFamily{*g}, c, stream);
}

// Inconsistent lists or a graph no kernel covers: FloodFamily::launch refuses them (LDPC_EHIP).  The
// staging buffers live in the workspace, so this form holds decode_entry's two locks itself, from
// the staging to the copies back, and goes through soft_launch under them.
int ldpc_bp_decode_batch(const int32_t *variable_to_check_list, const int32_t *check_to_variable_list, int n, int k,
                         int dv, int dc, const float *llr, int B, int max_iters, int algo, float alpha,
                         int early_stop, float *post, uint8_t *hard, int32_t *its) {
    LDPC_REQUIRE((B == 0 || llr) && B >= 0, "bad soft batch arguments");
    LDPC_REQUIRE(algo == LDPC_ALGO_SPA || algo == LDPC_ALGO_MINSUM, "algo must be LDPC_ALGO_SPA or LDPC_ALGO_MINSUM");
    ldpc_graph *g = nullptr;
    LDPC_TRY(ldpc_graph_create(variable_to_check_list, check_to_variable_list, n, k, dv, dc, &g));
    const OwnedGraph owner(g, ldpc_graph_destroy);
    if (B == 0) return LDPC_OK;  // validated graph, nothing to decode
    std::lock_guard<std::mutex> lk(g_mu);
    Workspace &ws = workspace(nullptr);
    std::lock_guard<std::mutex> wl(ws.mu);
    const size_t nb = (size_t)B * n;
    float *dl = ws.llr.get<float>(nb), *dp = ws.post.get<float>(nb);
    uint8_t *dh = ws.hard.get<uint8_t>(nb);
    int32_t *di = ws.itsb.get<int32_t>((size_t)B + 1);
    LDPC_ALLOCATED(dl && dp && dh && di);
    LDPC_HIP(hipMemcpy(dl, llr, nb * 4, hipMemcpyHostToDevice));
    const SoftCall c = decode_call(B, max_iters, algo, alpha, early_stop, dl, post ? dp : nullptr, dh, di);
    LDPC_TRY(soft_launch(ws, FloodFamily{*g}, c, nullptr));
    LDPC_HIP(hipDeviceSynchronize());
    if (post) LDPC_HIP(hipMemcpy(post, dp, nb * 4, hipMemcpyDeviceToHost));
    if (hard) LDPC_HIP(hipMemcpy(hard, dh, nb, hipMemcpyDeviceToHost));
    if (its) LDPC_HIP(hipMemcpy(its, di, (size_t)B * 4, hipMemcpyDeviceToHost));
    return LDPC_OK;
}

// --------------------------- channels / MC ---------------------------------
static int channel_params(int channel, float param, float *p, float *p2) {
    LDPC_REQUIRE(channel >= 0 && channel <= 2, "channel must be LDPC_CH_BEC, LDPC_CH_BSC or LDPC_CH_AWGN");
    *p = param;
    *p2 = 0.0f;
    if (channel == LDPC_CH_BSC) {
        LDPC_REQUIRE(param > 0.0f && param < 0.5f, "BSC crossover probability must be in (0, 0.5)");
        *p2 = (float)std::log((1.0 - (double)param) / (double)param);
    } else if (channel == LDPC_CH_AWGN) {
        LDPC_REQUIRE(param > 0.0f, "AWGN sigma must be > 0");
        *p2 = (float)(2.0 / ((double)param * (double)param));
    } else {
        LDPC_REQUIRE(param >= 0.0f && param <= 1.0f, "erasure probability must be in [0, 1]");
    }
    return LDPC_OK;
}

int ldpc_channel_dev(int channel, float param, uint64_t seed, uint64_t first_cw, int n, int B, void *d_out,
                     void *stream) {
    LDPC_REQUIRE((B == 0 || d_out) && n > 0 && B >= 0, "bad channel arguments");
    float p, p2;
    LDPC_TRY(channel_params(channel, param, &p, &p2));
    if (B == 0) return LDPC_OK;
    LDPC_HIP(launch_channel(channel, p, p2, seed, first_cw, n, B, d_out, static_cast<hipStream_t>(stream)));
    return LDPC_OK;
}

int ldpc_mc_batch_dev(const ldpc_graph *g, int channel, float param, uint64_t seed, uint64_t first_cw, int B,
                      int max_iters, int algo, float alpha, int early_stop, int expurgation,
                      int64_t stop_frame_errors, int64_t *d_counters, void *stream) {
    LDPC_REQUIRE(g && d_counters && B >= 0 && max_iters >= 0, "bad MC arguments");
    float p, p2;
    LDPC_TRY(channel_params(channel, param, &p, &p2));
    if (channel != LDPC_CH_BEC) {
        LDPC_REQUIRE(algo == LDPC_ALGO_SPA || algo == LDPC_ALGO_MINSUM, "bad algo");
        LDPC_REQUIRE(g->consistent, "soft decoding needs consistent edge lists");
    }
    if (B == 0) return LDPC_OK;
    const SoftCall c = mc_call(B, max_iters, algo, alpha, early_stop, make_chan(channel, p, p2, seed), first_cw);
    if (channel != LDPC_CH_BEC)
        return mc_entry(c, expurgation, stop_frame_errors, d_counters, stream, soft_decode(FloodFamily{*g}));
    return mc_entry(c, expurgation, stop_frame_errors, d_counters, stream,
                    [&](Workspace &, const SoftCall &mc, hipStream_t s) {  // exact erasure decoding (bec.hip)
                        LDPC_HIP(launch_mc_bec(*g, p, p2, seed, first_cw, B, max_iters, mc.trial, mc.its, s));
                        return (int)LDPC_OK;
                    });
}

// --------------------------- Gallager A/B (gb.hip) -------------------------
// The checks the two Gallager entries share: LDPC_EINVAL for bad arguments, LDPC_EUNSUP for a
// variable degree beyond the four count planes or planes that fit LDS at no plane word
static int gb_check(const ldpc_graph *g, int B, int max_iters, int b, bool es, bool mc, GbPlan &plan) {
    LDPC_REQUIRE(g && B >= 0 && max_iters >= 0, "bad Gallager A/B arguments");
    LDPC_REQUIRE(b >= 0 && b <= kGbMaxB, "flip threshold b must be 0 (Gallager A) .. 14");
    LDPC_REQUIRE(g->consistent,
                 "Gallager decoding needs consistent edge lists (each (v,c) pair listed equally often on both sides)");
    if (g->max_vdeg > kGbMaxVdeg) {
        set_error("Gallager A/B counts disagreements in four planes: variable degrees up to 15");
        return LDPC_EUNSUP;
    }
    plan = gb_plan(g->n, g->E, B, max_iters, es, mc);
    if (!plan.threads) {
        set_error("the Gallager A/B planes (one word per slot and variable) fit LDS at no plane word");
        return LDPC_EUNSUP;
    }
    return LDPC_OK;
}

int ldpc_gb_decode_batch_dev(const ldpc_graph *g, const uint8_t *d_bits, int B, int max_iters, int b, int early_stop,
                             uint8_t *d_hard, int32_t *d_its, void *stream) {
    GbPlan plan;
    LDPC_TRY(gb_check(g, B, max_iters, b, early_stop != 0, false, plan));
    LDPC_REQUIRE(B == 0 || d_bits, "null received bits");
    if (B == 0) return LDPC_OK;
    LDPC_HIP(launch_gb_decode(plan, *g, d_bits, B, max_iters, b, early_stop != 0, d_hard, d_its,
                              static_cast<hipStream_t>(stream)));
    return LDPC_OK;
}

int ldpc_mc_gb_batch_dev(const ldpc_graph *g, float p, uint64_t seed, uint64_t first_cw, int B, int max_iters, int b,
                         int early_stop, int expurgation, int64_t stop_frame_errors, int64_t *d_counters,
                         void *stream) {
    GbPlan plan;
    LDPC_TRY(gb_check(g, B, max_iters, b, early_stop != 0, true, plan));
    LDPC_REQUIRE(d_counters, "null counters");
    float cp, cp2;
    LDPC_TRY(channel_params(LDPC_CH_BSC, p, &cp, &cp2));
    if (B == 0) return LDPC_OK;
    const SoftCall c = mc_call(B, max_iters, 0, 1.0f, early_stop, make_chan(LDPC_CH_BSC, cp, cp2, seed), first_cw);
    return mc_entry(c, expurgation, stop_frame_errors, d_counters, stream,
                    [&](Workspace &, const SoftCall &mc, hipStream_t s) {
                        LDPC_HIP(launch_mc_gb(plan, *g, mc.ch, mc.first_cw, B, max_iters, b, mc.early_stop, mc.trial,
                                              mc.its, s));
                        return (int)LDPC_OK;
                    });
}

// The launch plans (gb_plan) of `count` Gallager A/B calls on a graph of n variables and E slots,
// from the shape alone.  calls[i] = {B, iters, early_stop, mc}; out + 8 i = {threads, W, plane
// bytes, codewords per workgroup, grid, LDS bytes, LDS cap, scratch bytes}; names + 64 i: the
// kernel's display name.  A call whose planes fit at no plane word is a row of zeros named "none".
int ldpc_debug_gb_plan(int n, int E, int count, const int32_t *calls, int64_t *out, char *names) {
    LDPC_REQUIRE(n > 0 && E > 0 && count >= 0 && (count == 0 || (calls && out && names)), "bad plan arguments");
    for (int i = 0; i < count; ++i) {
        const int32_t *c = calls + 4 * (size_t)i;
        LDPC_REQUIRE(c[0] >= 0 && c[1] >= 0, "bad plan arguments");
        const GbPlan p = gb_plan(n, E, c[0], c[1], c[2] != 0, c[3] != 0);
        int64_t *o = out + 8 * (size_t)i;
        o[0] = p.threads; o[1] = p.W; o[2] = p.plane; o[3] = p.cw_per_wg; o[4] = p.grid; o[5] = (int64_t)p.lds;
        o[6] = (int64_t)p.cap; o[7] = (int64_t)p.scratch;
        snprintf(names + 64 * (size_t)i, 64, "%s", p.name);
    }
    return LDPC_OK;
}

// --------------------------- layered schedule ------------------------------
// The argument checks the two layered entries share; LDPC_EUNSUP for a graph without a schedule
static int layered_check(const ldpc_graph *g, int algo) {
    LDPC_REQUIRE(algo == LDPC_ALGO_SPA || algo == LDPC_ALGO_MINSUM, "algo must be LDPC_ALGO_SPA or LDPC_ALGO_MINSUM");
    LDPC_REQUIRE(g->consistent,
                 "soft decoding needs consistent edge lists (each (v,c) pair listed equally often on both sides)");
    if (g->lay_L <= 0) {
        set_error(kNoSchedule);
        return LDPC_EUNSUP;
    }
    return LDPC_OK;
}

int ldpc_bp_layered_decode_batch_dev(const ldpc_graph *g, const float *d_llr, int B, int max_iters, int algo,
                                     float alpha, int early_stop, float *d_post, uint8_t *d_hard, int32_t *d_its,
                                     void *stream) {
    LDPC_REQUIRE(g && (B == 0 || d_llr) && B >= 0 && max_iters >= 0, "bad soft batch arguments");
    LDPC_TRY(layered_check(g, algo));
    if (B == 0) return LDPC_OK;
    const SoftCall c = decode_call(B, max_iters, algo, alpha, early_stop, d_llr, d_post, d_hard, d_its);
    return decode_entry(LayerFamily{*g}, c, stream);
}

int ldpc_mc_layered_batch_dev(const ldpc_graph *g, int channel, float param, uint64_t seed, uint64_t first_cw, int B,
                              int max_iters, int algo, float alpha, int early_stop, int expurgation,
                              int64_t stop_frame_errors, int64_t *d_counters, void *stream) {
    LDPC_REQUIRE(g && d_counters && B >= 0 && max_iters >= 0, "bad MC arguments");
    LDPC_REQUIRE(channel != LDPC_CH_BEC, "the layered schedule decodes the BSC and the BI-AWGN channel (BEC: ldpc_mc_batch_dev)");
    float p, p2;
    LDPC_TRY(channel_params(channel, param, &p, &p2));
    LDPC_TRY(layered_check(g, algo));
    if (B == 0) return LDPC_OK;
    const SoftCall c = mc_call(B, max_iters, algo, alpha, early_stop, make_chan(channel, p, p2, seed), first_cw);
    return mc_entry(c, expurgation, stop_frame_errors, d_counters, stream, soft_decode(LayerFamily{*g}));
}

const char *ldpc_layer_rule(void) { return kLayerRule; }

int ldpc_debug_layer_schedule(const int32_t *check_ptr, const int32_t *check_var, const int32_t *var_ptr,
                              const int32_t *var_slot, int n, int m, int32_t *num_layers, int32_t *layer) {
    LDPC_REQUIRE(num_layers, "null num_layers");
    HostGraph h;
    LDPC_TRY(host_graph_from_csr(check_ptr, check_var, var_ptr, var_slot, n, m, h));
    LayerSchedule S;
    if (!build_layer_schedule(h, S)) {
        set_error(kNoSchedule);
        return LDPC_EUNSUP;
    }
    *num_layers = S.L;
    if (layer) std::copy(S.layer.begin(), S.layer.end(), layer);
    return LDPC_OK;
}

int ldpc_debug_layer_plan(const int32_t *check_ptr, const int32_t *check_var, const int32_t *var_ptr,
                          const int32_t *var_slot, int n, int m, int count, const int32_t *calls, int cus, int64_t *out,
                          char *names) {
    return graph_plans(check_ptr, check_var, var_ptr, var_slot, n, m, count, calls, cus, out, names, bp_layer_plan,
                       true, &BpPlan::lds_slots);
}

// --------------------------- fixed-point layered min-sum -------------------
int ldpc_quant_check(const ldpc_quant *q) {
    LDPC_REQUIRE(q, "null ldpc_quant");
    LDPC_REQUIRE(q->msg_bits >= 2 && q->msg_bits <= 7, "ldpc_quant: need 2 <= msg_bits <= 7");
    LDPC_REQUIRE(q->post_bits >= q->msg_bits && q->post_bits <= 8, "ldpc_quant: need msg_bits <= post_bits <= 8");
    LDPC_REQUIRE(q->norm8 >= 1 && q->norm8 <= 8, "ldpc_quant: need 1 <= norm8 <= 8");
    LDPC_REQUIRE(q->offset >= 0 && q->offset <= (1 << (q->msg_bits - 1)) - 1, "ldpc_quant: need 0 <= offset <= Q");
    LDPC_REQUIRE(std::isfinite(q->scale) && q->scale > 0.0f, "ldpc_quant: scale must be finite and > 0");
    return LDPC_OK;
}

// The checks the two fixed-point entries share; LDPC_EUNSUP for a graph without a schedule or
// with a block beyond LDS
static int layered_q_check(const ldpc_graph *g, const ldpc_quant *q, int B, int max_iters, bool mc, bool cw = false) {
    LDPC_TRY(ldpc_quant_check(q));
    LDPC_TRY(layered_check(g, LDPC_ALGO_MINSUM));
    if (bp_layer_q_cw_plan(*g, B, max_iters, mc, cw).path == BpPath::None) {
        set_error(cw ? "the fixed-point layered block (posteriors, check records and the codeword's bit plane) does not fit LDS"
                         : "the fixed-point layered block (posteriors and check records) does not fit LDS");
        return LDPC_EUNSUP;
    }
    return LDPC_OK;
}

int ldpc_bp_layered_q_decode_batch_dev(const ldpc_graph *g, const float *d_llr, int B, int max_iters,
                                       const ldpc_quant *q, int early_stop, int8_t *d_post, uint8_t *d_hard,
                                       int32_t *d_its, void *stream) {
    LDPC_REQUIRE(g && (B == 0 || d_llr) && B >= 0 && max_iters >= 0, "bad soft batch arguments");
    LDPC_TRY(layered_q_check(g, q, B, max_iters, false));
    if (B == 0) return LDPC_OK;
    const SoftCall c = decode_call(B, max_iters, LDPC_ALGO_MINSUM, 1.0f, early_stop, d_llr, d_post, d_hard, d_its);
    return decode_entry(LayerQFamily{*g, *q}, c, stream);
}

int ldpc_mc_layered_q_batch_dev(const ldpc_graph *g, int channel, float param, uint64_t seed, uint64_t first_cw,
                                int B, int max_iters, const ldpc_quant *q, int early_stop, int expurgation,
                                int64_t stop_frame_errors, int64_t *d_counters, void *stream) {
    LDPC_REQUIRE(g && d_counters && B >= 0 && max_iters >= 0, "bad MC arguments");
    LDPC_REQUIRE(channel != LDPC_CH_BEC, "the layered schedule decodes the BSC and the BI-AWGN channel (BEC: ldpc_mc_batch_dev)");
    float p, p2;
    LDPC_TRY(channel_params(channel, param, &p, &p2));
    LDPC_TRY(layered_q_check(g, q, B, max_iters, true));
    if (B == 0) return LDPC_OK;
    const SoftCall c =
        mc_call(B, max_iters, LDPC_ALGO_MINSUM, 1.0f, early_stop, make_chan(channel, p, p2, seed), first_cw);
    return mc_entry(c, expurgation, stop_frame_errors, d_counters, stream, soft_decode(LayerQFamily{*g, *q}));
}

static const char *const kNoCwPlan =
    "no plan in the codeword mode: not a Monte-Carlo call, or the block with the codeword's bit plane does not fit LDS";

int ldpc_mc_layered_q_cw_batch_dev(const ldpc_graph *g, const ldpc_rate_match *rm, const uint8_t *d_cw, int channel,
                                   float param, float known_llr, uint64_t seed, uint64_t first_cw, int B,
                                   int max_iters, const ldpc_quant *q, int early_stop, int expurgation,
                                   int64_t stop_frame_errors, int64_t *d_counters, void *stream) {
    LDPC_REQUIRE(g && d_counters && B >= 0 && max_iters >= 0, "bad MC arguments");
    LDPC_REQUIRE(channel != LDPC_CH_BEC, "the layered schedule decodes the BSC and the BI-AWGN channel (BEC: ldpc_mc_batch_dev)");
    float p, p2;
    LDPC_TRY(channel_params(channel, param, &p, &p2));
    LDPC_TRY(layered_q_check(g, q, B, max_iters, true, true));
    if (rm) {
        LDPC_REQUIRE(rm->n == g->n, "the rate-matching description is of another n than the graph");
        LDPC_REQUIRE(rm->n_known == 0 || (std::isfinite(known_llr) && known_llr > 0.0f),
                     "known_llr must be finite and > 0");
    }
    if (B == 0) return LDPC_OK;
    SoftCall c = mc_call(B, max_iters, LDPC_ALGO_MINSUM, 1.0f, early_stop, make_chan(channel, p, p2, seed), first_cw);
    c.cw_mode = true, c.cw = d_cw, c.rm = rm ? rm->desc : nullptr, c.known_llr = known_llr;
    return mc_entry(c, expurgation, stop_frame_errors, d_counters, stream, soft_decode(LayerQFamily{*g, *q}));
}

int ldpc_debug_layer_q_cw_plan(const int32_t *check_ptr, const int32_t *check_var, const int32_t *var_ptr,
                               const int32_t *var_slot, int n, int m, int count, const int32_t *calls, int cus,
                               int has_desc, int64_t *out, char *names) {
    (void)has_desc;  // the count mask is re-read from the description: no LDS of its own
    return graph_plans(check_ptr, check_var, var_ptr, var_slot, n, m, count, calls, cus, out, names,
                       [](const GraphShape &g, int B, int iters, int, bool, bool mc, bool, int) {
                           return bp_layer_q_cw_plan(g, B, iters, mc, true);
                       },
                       true, &BpPlan::wg_per_cu, kNoCwPlan);
}

int ldpc_debug_layer_q_plan(const int32_t *check_ptr, const int32_t *check_var, const int32_t *var_ptr,
                            const int32_t *var_slot, int n, int m, int count, const int32_t *calls, int cus, int64_t *out,
                            char *names) {
    return graph_plans(check_ptr, check_var, var_ptr, var_slot, n, m, count, calls, cus, out, names, bp_layer_q_plan,
                       true, &BpPlan::wg_per_cu);
}

// --------------------------- quasi-cyclic codes, host only -----------------
int ldpc_debug_qc_expand(int mb, int nb, int Z, const int32_t *base, int32_t *check_ptr, int32_t *check_var,
                         int32_t *var_ptr, int32_t *var_slot, int32_t *layer) {
    HostGraph h;
    QcCode qc;
    LDPC_TRY(host_graph_from_qc(mb, nb, Z, base, h, qc));
    GraphShape g;
    HostLayouts L;
    LayoutOptions opt = layout_options();
    opt.qc = &qc;
    host_layouts(h, g, L, true, opt);
    if (g.lay_L <= 0) {
        set_error(kNoSchedule);
        return LDPC_EUNSUP;
    }
    if (check_ptr) std::copy(h.cptr.begin(), h.cptr.end(), check_ptr);
    if (check_var) std::copy(h.cvar.begin(), h.cvar.end(), check_var);
    if (var_ptr) std::copy(h.vptr.begin(), h.vptr.end(), var_ptr);
    if (var_slot) std::copy(h.vslot.begin(), h.vslot.end(), var_slot);
    if (layer) std::copy(L.lay.layer.begin(), L.lay.layer.end(), layer);
    return LDPC_OK;
}

// cw: bp_layer_q_cw_plan's (false: ldpc_debug_qc_plan)
static int qc_plans(int mb, int nb, int Z, const int32_t *base, int count, const int32_t *calls, int cus, bool cw,
                    int64_t *out, char *names) {
    LDPC_REQUIRE(count >= 0 && (count == 0 || (calls && out && names)) && cus > 0, "bad plan arguments");
    HostGraph h;
    QcCode qc;
    LDPC_TRY(host_graph_from_qc(mb, nb, Z, base, h, qc));
    GraphShape g;
    HostLayouts L;
    LayoutOptions opt = layout_options();
    opt.qc = &qc;
    host_layouts(h, g, L, true, opt);
    if (g.lay_L <= 0) {
        set_error(kNoSchedule);
        return LDPC_EUNSUP;
    }
    return write_plans(count, calls, out, names, &BpPlan::wg_per_cu, cw ? kNoCwPlan : nullptr,
                       [&](int B, int iters, int algo, bool et, bool mc, bool want_post) {
                           if (cw) return bp_layer_q_cw_plan(g, B, iters, mc, true);
                           return bp_layer_q_plan(g, B, iters, algo, et, mc, want_post, cus);
                       });
}

int ldpc_debug_qc_plan(int mb, int nb, int Z, const int32_t *base, int count, const int32_t *calls, int cus,
                       int64_t *out, char *names) {
    return qc_plans(mb, nb, Z, base, count, calls, cus, false, out, names);
}

int ldpc_debug_qc_cw_plan(int mb, int nb, int Z, const int32_t *base, int count, const int32_t *calls, int cus,
                          int has_desc, int64_t *out, char *names) {
    (void)has_desc;  // as ldpc_debug_layer_q_cw_plan
    return qc_plans(mb, nb, Z, base, count, calls, cus, true, out, names);
}

// --------------------------- random graphs / ensemble MC -------------------
static int check_regular_shape(int n, int dv, int dc) {
    LDPC_REQUIRE(n > 0 && dv > 0 && dc > 1 && (long)n * dv % dc == 0 && (long)n * dv < (1L << 30),
                 "need n*dv divisible by dc (regular configuration model)");
    return LDPC_OK;
}

// The regular sampler of both forms and of the ensemble Monte-Carlo (trial b decodes on graph b):
// search control from the (locked) workspace, then the launch into the caller's device lists or
// -- with none given -- into the workspace's own (chk, var).
static int sample_regular_locked(Workspace &ws, int n, int dv, int dc, uint64_t seed, uint64_t first_graph, int G,
                                 int32_t *&chk, int32_t *&var, int32_t *d_attempts, hipStream_t s) {
    if (!chk) {
        chk = ws.gchk.get<int32_t>((size_t)n * dv * G);
        var = ws.gvar.get<int32_t>((size_t)n * dv * G);
    }
    uint32_t *ctl = ws.sctl.get<uint32_t>(sample_ctl_words(G));
    LDPC_ALLOCATED(chk && var && ctl);
    LDPC_HIP(launch_sample_regular(n, dv, dc, seed, first_graph, G, chk, var, d_attempts, 1 << 20, ctl, s));
    return LDPC_OK;
}

int ldpc_sample_regular_dev(int n, int dv, int dc, uint64_t seed, uint64_t first_graph, int G,
                            int32_t *d_check_lookup, int32_t *d_variable_lookup, int32_t *d_attempts, void *stream) {
    LDPC_TRY(check_regular_shape(n, dv, dc));
    LDPC_REQUIRE(d_check_lookup && d_variable_lookup && G >= 0, "bad sampler arguments");
    LDPC_TRY(require_device());
    Workspace &ws = workspace(stream);
    std::lock_guard<std::mutex> wl(ws.mu);
    return sample_regular_locked(ws, n, dv, dc, seed, first_graph, G, d_check_lookup, d_variable_lookup, d_attempts,
                                 static_cast<hipStream_t>(stream));
}

int ldpc_debug_seq_stats(uint64_t *out, int reset) {
    LDPC_REQUIRE(out, "null output");
    LDPC_TRY(require_device());
    const hipError_t e = seq_stats(out, reset);
    if (e == hipErrorNotSupported) {
        set_error("sampler statistics need a -DLDPC_SEQ_STATS=1 build");
        return LDPC_EUNSUP;
    }
    LDPC_HIP(e);
    return LDPC_OK;
}

int ldpc_debug_peel_stats(uint64_t *out, int reset) {
    LDPC_REQUIRE(out, "null output");
    LDPC_TRY(require_device());
    LDPC_HIP(peel_stats(out, reset));
    return LDPC_OK;
}

int ldpc_debug_peel_cap(int F) {
    peel_cap(F);
    return LDPC_OK;
}

// The host sampler forms' way back: wait, then G graphs of E slots each and their attempt counts
static int sampled_to_host(const int32_t *chk, const int32_t *var, const int32_t *att, size_t E, int G,
                           int32_t *h_chk, int32_t *h_var, int32_t *h_att) {
    LDPC_HIP(hipDeviceSynchronize());
    LDPC_HIP(hipMemcpy(h_chk, chk, E * G * 4, hipMemcpyDeviceToHost));
    LDPC_HIP(hipMemcpy(h_var, var, E * G * 4, hipMemcpyDeviceToHost));
    if (h_att) LDPC_HIP(hipMemcpy(h_att, att, (size_t)G * 4, hipMemcpyDeviceToHost));
    return LDPC_OK;
}

int ldpc_sample_regular(int n, int dv, int dc, uint64_t seed, uint64_t first_graph, int G, int32_t *check_lookup,
                        int32_t *variable_lookup, int32_t *attempts) {
    LDPC_TRY(check_regular_shape(n, dv, dc));
    LDPC_REQUIRE(check_lookup && variable_lookup && G >= 0, "bad sampler arguments");
    LDPC_TRY(require_device());
    std::lock_guard<std::mutex> lk(g_mu);
    Workspace &ws = workspace(nullptr);
    std::lock_guard<std::mutex> wl(ws.mu);
    int32_t *chk = nullptr, *var = nullptr, *att = ws.gatt.get<int32_t>((size_t)G + 1);
    LDPC_ALLOCATED(att);
    LDPC_TRY(sample_regular_locked(ws, n, dv, dc, seed, first_graph, G, chk, var, att, nullptr));
    return sampled_to_host(chk, var, att, (size_t)n * dv, G, check_lookup, variable_lookup, attempts);
}

// Irregular configuration model: degree structure (host arrays) -> device shape buffer
// [vsock E | cptr m+1 | vptr n+1] on the workspace of `stream` (caller holds g_mu).
struct CsrShape {
    int E = 0, max_cdeg = 0, max_vdeg = 0;
    const int32_t *vsock = nullptr, *cptr = nullptr, *vptr = nullptr;
};
static int csr_shape_upload(int n, int m, const int32_t *var_ptr, const int32_t *check_ptr, Workspace &ws,
                            hipStream_t stream, CsrShape &out) {
    LDPC_REQUIRE(n > 0 && m > 0 && var_ptr && check_ptr, "bad degree structure");
    LDPC_REQUIRE(var_ptr[0] == 0 && check_ptr[0] == 0, "var_ptr / check_ptr must start at 0");
    for (int v = 0; v < n; ++v) {
        LDPC_REQUIRE(var_ptr[v + 1] >= var_ptr[v], "var_ptr must be non-decreasing");
        out.max_vdeg = std::max(out.max_vdeg, var_ptr[v + 1] - var_ptr[v]);
    }
    for (int c = 0; c < m; ++c) {
        LDPC_REQUIRE(check_ptr[c + 1] >= check_ptr[c], "check_ptr must be non-decreasing");
        out.max_cdeg = std::max(out.max_cdeg, check_ptr[c + 1] - check_ptr[c]);
    }
    const int E = var_ptr[n];
    LDPC_REQUIRE(E > 0 && E == check_ptr[m], "socket counts differ: var_ptr[n] != check_ptr[m]");
    std::vector<int32_t> h((size_t)E + m + 1 + n + 1);
    for (int v = 0; v < n; ++v)
        for (int e = var_ptr[v]; e < var_ptr[v + 1]; ++e) h[e] = v;
    std::copy(check_ptr, check_ptr + m + 1, h.begin() + E);
    std::copy(var_ptr, var_ptr + n + 1, h.begin() + E + m + 1);
    // an earlier sampler launch on this stream may still read the shape buffer
    LDPC_HIP(hipStreamSynchronize(stream));
    const int32_t *base = ws.shape.get<int32_t>(h.size());
    LDPC_ALLOCATED(base);
    LDPC_HIP(hipMemcpy(ws.shape.p, h.data(), h.size() * 4, hipMemcpyHostToDevice));
    out.E = E;
    out.vsock = base, out.cptr = base + E, out.vptr = base + E + m + 1;
    return LDPC_OK;
}

// The irregular sampler of both forms: the shape into the (locked) workspace, then the launch
// into the caller's device lists, or -- with none given -- into the workspace's own (chk, var, att).
static int sample_csr_locked(Workspace &ws, int n, int m, const int32_t *var_ptr, const int32_t *check_ptr,
                             uint64_t seed, uint64_t first_graph, int G, int32_t *&chk, int32_t *&var, int32_t *&att,
                             hipStream_t s, CsrShape &sh) {
    LDPC_TRY(csr_shape_upload(n, m, var_ptr, check_ptr, ws, s, sh));
    if (!chk) {
        chk = ws.gchk.get<int32_t>((size_t)sh.E * G);
        var = ws.gvar.get<int32_t>((size_t)sh.E * G);
        att = ws.gatt.get<int32_t>((size_t)G + 1);
        LDPC_ALLOCATED(att);
    }
    uint32_t *ctl = ws.sctl.get<uint32_t>(sample_ctl_words(G));
    LDPC_ALLOCATED(chk && var && ctl);
    LDPC_HIP(launch_sample_csr(n, m, sh.E, sh.vsock, sh.cptr, sh.vptr, sh.max_cdeg, sh.max_vdeg, seed, first_graph, G,
                               chk, var, att, 1 << 20, ctl, s));
    return LDPC_OK;
}

int ldpc_sample_csr_dev(int n, int m, const int32_t *var_ptr, const int32_t *check_ptr, uint64_t seed,
                        uint64_t first_graph, int G, int32_t *d_check_var, int32_t *d_var_slot, int32_t *d_attempts,
                        void *stream) {
    LDPC_REQUIRE(d_check_var && d_var_slot && G >= 0, "bad sampler arguments");
    LDPC_TRY(require_device());
    std::lock_guard<std::mutex> lk(g_mu);
    Workspace &ws = workspace(stream);
    std::lock_guard<std::mutex> wl(ws.mu);
    CsrShape sh;
    return sample_csr_locked(ws, n, m, var_ptr, check_ptr, seed, first_graph, G, d_check_var, d_var_slot, d_attempts,
                             static_cast<hipStream_t>(stream), sh);
}

int ldpc_sample_csr(int n, int m, const int32_t *var_ptr, const int32_t *check_ptr, uint64_t seed,
                    uint64_t first_graph, int G, int32_t *check_var, int32_t *var_slot, int32_t *attempts) {
    LDPC_REQUIRE(check_var && var_slot && G >= 0, "bad sampler arguments");
    LDPC_TRY(require_device());
    std::lock_guard<std::mutex> lk(g_mu);
    Workspace &ws = workspace(nullptr);
    std::lock_guard<std::mutex> wl(ws.mu);
    CsrShape sh;
    int32_t *chk = nullptr, *var = nullptr, *att = nullptr;
    LDPC_TRY(sample_csr_locked(ws, n, m, var_ptr, check_ptr, seed, first_graph, G, chk, var, att, nullptr, sh));
    return sampled_to_host(chk, var, att, (size_t)sh.E, G, check_var, var_slot, attempts);
}

int ldpc_mc_ensemble_batch_dev(int n, int dv, int dc, int channel, float param, uint64_t seed, uint64_t first_cw,
                               int B, int max_iters, int expurgation, int64_t stop_frame_errors, int64_t *d_counters,
                               void *stream) {
    LDPC_TRY(check_regular_shape(n, dv, dc));
    LDPC_REQUIRE(channel == LDPC_CH_BEC, "ensemble Monte-Carlo is BEC-only (as parallel_simulator.py:168-272)");
    LDPC_REQUIRE(d_counters && B >= 0 && max_iters >= 0, "bad MC arguments");
    float p, p2;
    LDPC_TRY(channel_params(channel, param, &p, &p2));
    LDPC_TRY(require_device());
    if (B == 0) return LDPC_OK;
    const SoftCall c = mc_call(B, max_iters, 0, 1.0f, 0, make_chan(channel, p, p2, seed), first_cw);
    return mc_entry(c, expurgation, stop_frame_errors, d_counters, stream,
                    [&](Workspace &ws, const SoftCall &mc, hipStream_t s) {
                        int32_t *chk = nullptr, *var = nullptr;
                        LDPC_TRY(sample_regular_locked(ws, n, dv, dc, seed, first_cw, B, chk, var, nullptr, s));
                        LDPC_HIP(launch_mc_bec_ensemble(n, dv, dc, chk, var, p, seed, first_cw, B, max_iters, mc.trial,
                                                        mc.its, s));
                        return (int)LDPC_OK;
                    });
}

// --------------------------- ensemble soft decoding / MC -------------------
// The shape and mode checks the two ensemble soft entries share; LDPC_EUNSUP when no
// bp_ens_kernel covers the check degree.
static int ens_soft_check(int n, int dv, int dc, int algo) {
    LDPC_TRY(check_regular_shape(n, dv, dc));
    LDPC_REQUIRE(algo == LDPC_ALGO_SPA || algo == LDPC_ALGO_MINSUM, "algo must be LDPC_ALGO_SPA or LDPC_ALGO_MINSUM");
    if (bp_ens_plan(n, dv, dc, 1, 1, algo, false, false, true, 256).path == BpPath::None) {
        set_error("no ensemble soft kernel for this shape (check degree > 32)");
        return LDPC_EUNSUP;
    }
    return LDPC_OK;
}

// The launch plans (bp_ens_plan) of `count` ensemble soft-decoding calls on the (n, dv, dc)
// shape, host only; calls / out / names: write_plans'.  LDPC_EUNSUP (after filling out and names)
// when a call has no kernel.
int ldpc_debug_ens_plan(int n, int dv, int dc, int count, const int32_t *calls, int cus, int64_t *out, char *names) {
    LDPC_REQUIRE(count >= 0 && (count == 0 || (calls && out && names)) && cus > 0, "bad plan arguments");
    LDPC_TRY(check_regular_shape(n, dv, dc));
    return write_plans(count, calls, out, names, &BpPlan::lds_slots,
                       "no ensemble soft kernel for this call (check degree > 32, or a curve beyond LDS)",
                       [&](int B, int iters, int algo, bool et, bool mc, bool want_post) {
                           return bp_ens_plan(n, dv, dc, B, iters, algo, et, mc, want_post, cus);
                       });
}

int ldpc_bp_ensemble_decode_dev(int n, int dv, int dc, const int32_t *d_check_lookup, const int32_t *d_variable_lookup,
                                const float *d_llr, int B, int max_iters, int algo, float alpha, int early_stop,
                                float *d_post, uint8_t *d_hard, int32_t *d_its, void *stream) {
    LDPC_REQUIRE((B == 0 || (d_check_lookup && d_variable_lookup && d_llr)) && B >= 0 && max_iters >= 0,
                 "bad ensemble soft batch arguments");
    LDPC_TRY(ens_soft_check(n, dv, dc, algo));
    LDPC_TRY(require_device());
    if (B == 0) return LDPC_OK;
    const SoftCall c = decode_call(B, max_iters, algo, alpha, early_stop, d_llr, d_post, d_hard, d_its);
    return decode_entry(EnsFamily{n, dv, dc, d_check_lookup, d_variable_lookup}, c, stream);
}

int ldpc_mc_ensemble_soft_batch_dev(int n, int dv, int dc, int channel, float param, int algo, float alpha,
                                    int early_stop, uint64_t seed, uint64_t first_cw, int B, int max_iters,
                                    int expurgation, int64_t stop_frame_errors, int64_t *d_counters, void *stream) {
    if (channel == LDPC_CH_BEC)  // exact erasure decoding: algo, alpha and early_stop do not apply
        return ldpc_mc_ensemble_batch_dev(n, dv, dc, channel, param, seed, first_cw, B, max_iters, expurgation,
                                          stop_frame_errors, d_counters, stream);
    LDPC_REQUIRE(d_counters && B >= 0 && max_iters >= 0, "bad MC arguments");
    float p, p2;
    LDPC_TRY(channel_params(channel, param, &p, &p2));
    LDPC_TRY(ens_soft_check(n, dv, dc, algo));
    LDPC_TRY(require_device());
    if (B == 0) return LDPC_OK;
    const SoftCall c = mc_call(B, max_iters, algo, alpha, early_stop, make_chan(channel, p, p2, seed), first_cw);
    return mc_entry(c, expurgation, stop_frame_errors, d_counters, stream,
                    [&](Workspace &ws, const SoftCall &mc, hipStream_t s) {
                        // trial t: graph t (key = seed) and channel word t, as the BEC form
                        int32_t *chk = nullptr, *var = nullptr;
                        LDPC_TRY(sample_regular_locked(ws, n, dv, dc, seed, first_cw, B, chk, var, nullptr, s));
                        return soft_launch(ws, EnsFamily{n, dv, dc, chk, var}, mc, s);
                    });
}

// --------------------------- ML ("optimal") erasure decoding ---------------
static int ml_check_shape(int n, int m) {
    LDPC_REQUIRE(m >= 1 && m <= 1000, "ML decoding supports 1 <= n-k <= 1000 checks");
    LDPC_REQUIRE(n >= 1 && n <= 32767, "ML decoding supports n <= 32767");
    return LDPC_OK;
}

int ldpc_ml_decode_batch_dev(const ldpc_graph *g, const uint8_t *d_words, int B, uint8_t *d_out,
                             int32_t *d_unsolved, void *stream) {
    LDPC_REQUIRE(g && (B == 0 || (d_words && d_out && d_unsolved)) && B >= 0, "bad ML batch arguments");
    LDPC_TRY(ml_check_shape(g->n, g->m));
    if (B == 0) return LDPC_OK;
    LDPC_HIP(launch_ml_decode(g->cptr, g->cvar, 0, 0, g->n, g->m, d_words, B, d_out, d_unsolved,
                              static_cast<hipStream_t>(stream)));
    return LDPC_OK;
}

// The twin takes no lock and no workspace: it is this form's body
int ldpc_ml_decode_batch(const ldpc_graph *g, const uint8_t *words, int B, uint8_t *out, int32_t *unsolved) {
    LDPC_REQUIRE(g && (B == 0 || (words && out && unsolved)) && B >= 0, "bad ML batch arguments");
    LDPC_TRY(ml_check_shape(g->n, g->m));
    if (B == 0) return LDPC_OK;
    const size_t bytes = (size_t)B * g->n;
    std::lock_guard<std::mutex> lk(g_mu);
    Workspace &ws = workspace(nullptr);
    std::lock_guard<std::mutex> wl(ws.mu);
    uint8_t *dw = ws.mlw.get<uint8_t>(bytes), *dout = ws.mlo.get<uint8_t>(bytes);
    int32_t *du = ws.mlu.get<int32_t>(B);
    LDPC_ALLOCATED(dw && dout && du);
    LDPC_HIP(hipMemcpy(dw, words, bytes, hipMemcpyHostToDevice));
    LDPC_TRY(ldpc_ml_decode_batch_dev(g, dw, B, dout, du, nullptr));
    LDPC_HIP(hipDeviceSynchronize());
    LDPC_HIP(hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost));
    LDPC_HIP(hipMemcpy(unsolved, du, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost));
    return LDPC_OK;
}

int ldpc_ml_ensemble_decode_dev(int n, int dv, int dc, const int32_t *d_check_lookup, const uint8_t *d_words, int B,
                                uint8_t *d_out, int32_t *d_unsolved, void *stream) {
    LDPC_TRY(check_regular_shape(n, dv, dc));
    LDPC_REQUIRE((B == 0 || (d_check_lookup && d_words && d_out && d_unsolved)) && B >= 0, "bad ML batch arguments");
    LDPC_TRY(ml_check_shape(n, n * dv / dc));
    LDPC_TRY(require_device());
    if (B == 0) return LDPC_OK;
    LDPC_HIP(launch_ml_decode(nullptr, d_check_lookup, (int64_t)n * dv, dc, n, n * dv / dc, d_words, B, d_out,
                              d_unsolved, static_cast<hipStream_t>(stream)));
    return LDPC_OK;
}

int ldpc_mc_ml_batch_dev(const ldpc_graph *g, int n, int dv, int dc, float eps, uint64_t seed, uint64_t first_cw,
                         int B, int max_iters, int message_passing, int expurgation, int64_t stop_frame_errors,
                         int64_t *d_counters_mp, int64_t *d_counters_ml, void *stream) {
    LDPC_REQUIRE(d_counters_ml && B >= 0 && max_iters >= 0, "bad MC arguments");
    LDPC_REQUIRE(!message_passing || d_counters_mp, "message_passing needs d_counters_mp");
    float p, p2;
    LDPC_TRY(channel_params(LDPC_CH_BEC, eps, &p, &p2));
    const bool ens = (g == nullptr);
    if (ens) {
        LDPC_TRY(check_regular_shape(n, dv, dc));
        LDPC_TRY(require_device());
    } else {
        n = g->n;
    }
    const int m = ens ? n * dv / dc : g->m;
    LDPC_TRY(ml_check_shape(n, m));
    if (B == 0) return LDPC_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    Workspace &ws = workspace(stream);  // this (device, stream)'s lock only
    std::lock_guard<std::mutex> wl(ws.mu);
    uint8_t *dw = ws.mlw.get<uint8_t>((size_t)B * n), *dout = ws.mlo.get<uint8_t>((size_t)B * n);
    int32_t *du = ws.mlu.get<int32_t>(B), *cut = ws.cutoff.get<int32_t>(4), *chk = nullptr, *var = nullptr;
    LDPC_ALLOCATED(dw && dout && du && cut);
    if (ens) LDPC_TRY(sample_regular_locked(ws, n, dv, dc, seed, first_cw, B, chk, var, nullptr, s));
    // channel words of trials first_cw.. (the same Philox draws the fused BP kernels make)
    LDPC_HIP(launch_channel(LDPC_CH_BEC, p, p2, seed, first_cw, n, B, dw, s));
    if (ens)
        LDPC_HIP(launch_ml_decode(nullptr, chk, (int64_t)n * dv, dc, n, m, dw, B, dout, du, s));
    else
        LDPC_HIP(launch_ml_decode(g->cptr, g->cvar, 0, 0, n, m, dw, B, dout, du, s));
    if (message_passing) {
        int32_t *trial = ws.trial.get<int32_t>((size_t)B * (max_iters + 1)), *its = ws.its.get<int32_t>(B);
        LDPC_ALLOCATED(trial && its);
        if (ens)
            LDPC_HIP(launch_mc_bec_ensemble(n, dv, dc, chk, var, p, seed, first_cw, B, max_iters, trial, its, s));
        else
            LDPC_HIP(launch_mc_bec(*g, p, p2, seed, first_cw, B, max_iters, trial, its, s));
        // the stop rule counts message-passing frame errors (parallel_simulator.py:226-231)
        LDPC_HIP(launch_mc_reduce(trial, its, B, max_iters, expurgation, stop_frame_errors, d_counters_mp, cut, s));
        LDPC_HIP(launch_mc_reduce_cut(du, nullptr, B, 0, -1, cut, d_counters_ml, s));
    } else {
        // ML only: the stop rule counts ML frame errors (:240-241)
        LDPC_HIP(launch_mc_reduce(du, nullptr, B, 0, -1, stop_frame_errors, d_counters_ml, cut, s));
    }
    return LDPC_OK;
}

// --------------------------- codewords: encoder, info bits, channel, counts (encode.hip) ----------
// The handle of a description: the two tables on the current device, the positions kept on the host
static int device_encoder(const EncoderDesc &d, ldpc_encoder **out) {
    std::vector<uint32_t> At;
    std::vector<int32_t> src;
    encoder_device_tables(d, At, src);
    std::unique_ptr<ldpc_encoder, void (*)(ldpc_encoder *)> e(new ldpc_encoder(), ldpc_encoder_destroy);
    e->n = d.n, e->K = d.K, e->rank = d.rank, e->KW = d.KW;
    e->info_pos = d.info_pos, e->par_pos = d.par_pos;
    (void)hipGetDevice(&e->device);
    if (!At.empty()) {
        LDPC_HIP(hipMalloc(reinterpret_cast<void **>(&e->At), At.size() * 4));
        LDPC_HIP(hipMemcpy(e->At, At.data(), At.size() * 4, hipMemcpyHostToDevice));
    }
    LDPC_HIP(hipMalloc(reinterpret_cast<void **>(&e->src), src.size() * 4));
    LDPC_HIP(hipMemcpy(e->src, src.data(), src.size() * 4, hipMemcpyHostToDevice));
    *out = e.release();
    return LDPC_OK;
}

int ldpc_encoder_create(const ldpc_graph *g, ldpc_encoder **out) {
    LDPC_REQUIRE(g && out, "null graph / output handle");
    LDPC_TRY(require_device());
    HostGraph h;  // the slots of H, back from the device graph: all the elimination reads
    h.n = g->n, h.m = g->m;
    h.cptr.resize((size_t)g->m + 1);
    h.cvar.resize(g->E);
    LDPC_HIP(hipMemcpy(h.cptr.data(), g->cptr, h.cptr.size() * 4, hipMemcpyDeviceToHost));
    if (g->E) LDPC_HIP(hipMemcpy(h.cvar.data(), g->cvar, h.cvar.size() * 4, hipMemcpyDeviceToHost));
    EncoderDesc d;
    build_encoder(h, d);
    return device_encoder(d, out);
}

void ldpc_encoder_destroy(ldpc_encoder *e) {
    if (!e) return;
    (void)hipFree(e->At);
    (void)hipFree(e->src);
    delete e;
}

int ldpc_encoder_info(const ldpc_encoder *e, int32_t *n, int32_t *K, int32_t *rank) {
    LDPC_REQUIRE(e, "null encoder");
    if (n) *n = e->n;
    if (K) *K = e->K;
    if (rank) *rank = e->rank;
    return LDPC_OK;
}

int ldpc_encoder_positions(const ldpc_encoder *e, int32_t *info_pos, int32_t *par_pos) {
    LDPC_REQUIRE(e, "null encoder");
    if (info_pos) std::copy(e->info_pos.begin(), e->info_pos.end(), info_pos);
    if (par_pos) std::copy(e->par_pos.begin(), e->par_pos.end(), par_pos);
    return LDPC_OK;
}

const char *ldpc_encode_rule(void) { return kEncodeRule; }

int ldpc_debug_encoder_build(const int32_t *check_ptr, const int32_t *check_var, int n, int m, int32_t *rank,
                             int32_t *info_pos, int32_t *par_pos, uint32_t *A_words) {
    LDPC_REQUIRE(check_ptr && n > 0 && m > 0 && rank, "bad encoder arguments");
    LDPC_REQUIRE(check_ptr[0] == 0, "check_ptr must start at 0");
    for (int c = 0; c < m; ++c) LDPC_REQUIRE(check_ptr[c + 1] >= check_ptr[c], "check_ptr must not decrease");
    const int E = check_ptr[m];
    LDPC_REQUIRE(E == 0 || check_var, "null check_var");
    for (int s = 0; s < E; ++s) LDPC_REQUIRE(check_var[s] >= 0 && check_var[s] < n, "check_var outside [0, n)");
    HostGraph h;
    h.n = n, h.m = m;
    h.cptr.assign(check_ptr, check_ptr + m + 1);
    h.cvar.assign(check_var, check_var + E);
    EncoderDesc d;
    build_encoder(h, d);
    *rank = d.rank;
    if (info_pos) std::copy(d.info_pos.begin(), d.info_pos.end(), info_pos);
    if (par_pos) std::copy(d.par_pos.begin(), d.par_pos.end(), par_pos);
    if (A_words) std::copy(d.A.begin(), d.A.end(), A_words);
    return LDPC_OK;
}

// The launch plans (encode_plan) of `count` encode calls, from the shape alone.  calls[i] = {n, K,
// rank, B}; out + 9 i = {threads, W, codewords per workgroup, grid, LDS bytes, LDS cap, plane words
// per parity row, scratch bytes, grid of the write pass}; names + 64 i: the kernel's display name.
// LDPC_EUNSUP, after every row is filled, when some call's information planes fit LDS at no W (its
// row: zeros named "none").
int ldpc_debug_encode_plan(int count, const int32_t *calls, int64_t *out, char *names) {
    LDPC_REQUIRE(count >= 0 && (count == 0 || (calls && out && names)), "bad plan arguments");
    bool none = false;
    for (int i = 0; i < count; ++i) {
        const int32_t *c = calls + 4 * (size_t)i;
        LDPC_REQUIRE(c[0] > 0 && c[1] >= 0 && c[2] >= 0 && c[1] + c[2] == c[0] && c[3] >= 0, "bad plan arguments");
        const EncodePlan p = encode_plan(c[0], c[1], c[2], c[3]);
        int64_t *o = out + 9 * (size_t)i;
        o[0] = p.threads; o[1] = p.W; o[2] = p.cw_per_wg; o[3] = p.grid; o[4] = (int64_t)p.lds; o[5] = (int64_t)p.cap;
        o[6] = p.pwords; o[7] = (int64_t)p.scratch; o[8] = p.write_grid;
        snprintf(names + 64 * (size_t)i, 64, "%s", p.name);
        none |= !p.threads;
    }
    if (none) {
        set_error("the information planes (4 K bytes per 32 codewords) fit LDS at no tile width");
        return LDPC_EUNSUP;
    }
    return LDPC_OK;
}

int ldpc_encode_batch_dev(const ldpc_encoder *e, const uint8_t *d_info, int B, uint8_t *d_cw, void *stream) {
    LDPC_REQUIRE(e && B >= 0, "bad encode arguments");
    LDPC_REQUIRE(B == 0 || (d_cw && (d_info || e->K == 0)), "null information bits / codewords");
    if (B == 0) return LDPC_OK;
    const EncodePlan p = encode_plan(e->n, e->K, e->rank, B);
    if (!p.threads) {
        set_error("the information planes (4 K bytes per 32 codewords) fit LDS at no tile width");
        return LDPC_EUNSUP;
    }
    LDPC_REQUIRE(p.write_grid <= 0x7fffffff, "B * n beyond one launch: encode in smaller batches");
    std::lock_guard<std::mutex> lk(g_mu);
    Workspace &ws = workspace(stream);
    std::lock_guard<std::mutex> wl(ws.mu);
    uint32_t *planes = ws.scratch.get<uint32_t>(p.scratch / 4);
    LDPC_ALLOCATED(planes);
    LDPC_HIP(launch_encode(p, *e, d_info, B, planes, d_cw, static_cast<hipStream_t>(stream)));
    return LDPC_OK;
}

int ldpc_info_bits_dev(uint64_t seed, uint64_t first_cw, int K, int B, uint8_t *d_info, void *stream) {
    LDPC_REQUIRE(K >= 0 && B >= 0 && (B == 0 || K == 0 || d_info), "bad information-bit arguments");
    LDPC_REQUIRE(((int64_t)B * ((K + 3) / 4) + 255) / 256 <= 0x7fffffff, "B * K beyond one launch");
    LDPC_HIP(launch_info_bits(seed, first_cw, K, B, d_info, static_cast<hipStream_t>(stream)));
    return LDPC_OK;
}

int ldpc_channel_cw_dev(int channel, float param, uint64_t seed, uint64_t first_cw, int n, int B, const uint8_t *d_cw,
                        void *d_out, void *stream) {
    LDPC_REQUIRE((B == 0 || d_out) && n > 0 && B >= 0, "bad channel arguments");
    float p, p2;
    LDPC_TRY(channel_params(channel, param, &p, &p2));
    if (B == 0) return LDPC_OK;
    LDPC_HIP(launch_channel_cw(channel, p, p2, seed, first_cw, n, B, d_cw, d_out, static_cast<hipStream_t>(stream)));
    return LDPC_OK;
}

int ldpc_mc_cw_count_dev(const uint8_t *d_cw, const void *d_chan, int chan_is_llr, const uint8_t *d_hard,
                         const int32_t *d_its, int n, int B, int max_iters, int expurgation, int64_t stop_frame_errors,
                         int64_t *d_counters, void *stream) {
    LDPC_REQUIRE(d_counters && n > 0 && B >= 0 && max_iters >= 0, "bad MC arguments");
    LDPC_REQUIRE(B == 0 || (d_cw && d_chan && d_hard), "null codewords / channel outputs / decisions");
    if (B == 0) return LDPC_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    Workspace &ws = workspace(stream);  // this (device, stream)'s lock only, as mc_entry
    std::lock_guard<std::mutex> wl(ws.mu);
    int32_t *trial = ws.trial.get<int32_t>((size_t)B * (max_iters + 1)), *cut = ws.cutoff.get<int32_t>(4);
    LDPC_ALLOCATED(trial && cut);
    LDPC_HIP(launch_cw_count(d_cw, d_chan, chan_is_llr != 0, d_hard, n, B, max_iters, trial, s));
    LDPC_HIP(launch_mc_reduce(trial, d_its, B, max_iters, expurgation, stop_frame_errors, d_counters, cut, s));
    return LDPC_OK;
}

// --------------------------- rate matching (rate_match_host.cpp, rate_match.hip) -----------------
int ldpc_rate_match_create(int n, const uint8_t *cls, const uint8_t *count, ldpc_rate_match **out) {
    LDPC_REQUIRE(out, "null output handle");
    RateMatchDesc d;
    LDPC_TRY(rate_match_pack(n, cls, count, d));
    LDPC_TRY(require_device());
    std::unique_ptr<ldpc_rate_match, void (*)(ldpc_rate_match *)> rm(new ldpc_rate_match(), ldpc_rate_match_destroy);
    rm->n = d.n, rm->n_tx = d.n_tx, rm->n_punct = d.n_punct, rm->n_known = d.n_known, rm->n_count = d.n_count;
    (void)hipGetDevice(&rm->device);
    LDPC_HIP(hipMalloc(reinterpret_cast<void **>(&rm->desc), d.packed.size()));
    LDPC_HIP(hipMemcpy(rm->desc, d.packed.data(), d.packed.size(), hipMemcpyHostToDevice));
    *out = rm.release();
    return LDPC_OK;
}

void ldpc_rate_match_destroy(ldpc_rate_match *rm) {
    if (!rm) return;
    (void)hipFree(rm->desc);
    delete rm;
}

int ldpc_rate_match_info(const ldpc_rate_match *rm, int32_t *n, int32_t *n_tx, int32_t *n_punct, int32_t *n_known,
                         int32_t *n_count) {
    LDPC_REQUIRE(rm, "null rate-matching description");
    if (n) *n = rm->n;
    if (n_tx) *n_tx = rm->n_tx;
    if (n_punct) *n_punct = rm->n_punct;
    if (n_known) *n_known = rm->n_known;
    if (n_count) *n_count = rm->n_count;
    return LDPC_OK;
}

int ldpc_debug_rate_match_pack(int n, const uint8_t *cls, const uint8_t *count, uint8_t *packed, int32_t *info) {
    RateMatchDesc d;
    LDPC_TRY(rate_match_pack(n, cls, count, d));
    if (packed) std::copy(d.packed.begin(), d.packed.end(), packed);
    if (info) info[0] = d.n, info[1] = d.n_tx, info[2] = d.n_punct, info[3] = d.n_known, info[4] = d.n_count;
    return LDPC_OK;
}

int ldpc_channel_rm_dev(const ldpc_rate_match *rm, int channel, float param, float known_llr, uint64_t seed,
                        uint64_t first_cw, int B, const uint8_t *d_cw, void *d_out, void *stream) {
    LDPC_REQUIRE(rm, "null rate-matching description");
    LDPC_REQUIRE((B == 0 || d_out) && B >= 0, "bad channel arguments");
    LDPC_REQUIRE(std::isfinite(known_llr) && known_llr > 0.0f, "known_llr must be finite and > 0");
    float p, p2;
    LDPC_TRY(channel_params(channel, param, &p, &p2));
    if (B == 0) return LDPC_OK;
    LDPC_REQUIRE(((int64_t)B * ((rm->n + 3) / 4) + 255) / 256 <= 0x7fffffff, "B * n beyond one launch");
    LDPC_HIP(launch_channel_rm(rm->desc, channel, p, p2, known_llr, seed, first_cw, rm->n, B, d_cw, d_out,
                               static_cast<hipStream_t>(stream)));
    return LDPC_OK;
}

int ldpc_mc_rm_count_dev(const ldpc_rate_match *rm, const uint8_t *d_cw, const void *d_chan, int chan_kind,
                         const uint8_t *d_dec, const int32_t *d_its, int B, int max_iters, int expurgation,
                         int64_t stop_frame_errors, int64_t *d_counters, void *stream) {
    LDPC_REQUIRE(rm, "null rate-matching description");
    LDPC_REQUIRE(d_counters && B >= 0 && max_iters >= 0, "bad MC arguments");
    LDPC_REQUIRE(chan_kind >= 0 && chan_kind <= 2, "chan_kind must be 0 (BEC words), 1 (LLRs) or 2 (received bits)");
    LDPC_REQUIRE(B == 0 || (d_chan && d_dec), "null channel outputs / decisions");
    if (B == 0) return LDPC_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    Workspace &ws = workspace(stream);  // this (device, stream)'s lock only, as ldpc_mc_cw_count_dev
    std::lock_guard<std::mutex> wl(ws.mu);
    int32_t *trial = ws.trial.get<int32_t>((size_t)B * (max_iters + 1)), *cut = ws.cutoff.get<int32_t>(4);
    LDPC_ALLOCATED(trial && cut);
    LDPC_HIP(launch_rm_count(rm->desc, d_cw, d_chan, chan_kind, d_dec, rm->n, B, max_iters, trial, s));
    LDPC_HIP(launch_mc_reduce(trial, d_its, B, max_iters, expurgation, stop_frame_errors, d_counters, cut, s));
    return LDPC_OK;
}

}  // extern "C"
