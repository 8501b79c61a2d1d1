// mcbs_api.hip — host side of the C ABI declared in include/mcbs.h (libmcbs.so).
// One translation unit: the kernels are included below.  Build: marlon_amd/csrc/Makefile (hipcc, gfx950).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "mcbs.h"
#include "mcbs_device.h"
#include "mcbs_extents.h"
#include "mcbs_step.hip"
#include "mcbs_step_coop.hip"
#include "mcbs_obs.hip"
#include "mcbs_aux.hip"
#include "mcbs_defend.hip"
#include "mcbs_logits.hip"
#include "mcbs_packed_mask.hip"
#include "mcbs_categorical.hip"
#include "mcbs_categorical_grad.hip"
#include "mcbs_linear_categorical.hip"
#include "mcbs_linear_categorical_grad.hip"
#include "mcbs_multicategorical.hip"
#include "mcbs_gae.hip"
#include "mcbs_features.hip"
#include "mcbs_obs_packing.hip"
#include "mcbs_first_layer.hip"
#include "mcbs_wrapper_fused.hip"
#include "mcbs_two_agent.hip"
#include "mcbs_mask_keys.hip"
#include "mcbs_defender_obs_packing.hip"

using namespace mcbs;

static thread_local char g_err[512] = "";

// Calls that must address a particular device (allocation, synchronous copies) select it for their own duration only: the
// caller's current device (PyTorch's, in a single process driving several GPUs) is put back on every exit path.
struct DeviceGuard {
    int prev = -1;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != device) err = hipSetDevice(device); else prev = -1;
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

static int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                                     \
    do {                                                                                                  \
        hipError_t _e = (expr);                                                                           \
        if (_e != hipSuccess) return fail(MCBS_EHIP, "%s failed: %s", #expr, hipGetErrorString(_e));      \
    } while (0)

// Every entry point that launches on (or synchronises with) a batch's GPU runs with that GPU selected: a single process whose current
// device differs from the batch's (PyTorch driving several GPUs) would otherwise launch on the wrong device or fail with an invalid
// handle.  hipGetDevice is a thread-local read; hipSetDevice is only called when the devices differ, and the caller's device is put back.
#define MCBS_ON_DEVICE(b)                                                                                                      \
    DeviceGuard _dev_guard((b)->cfg.device);                                                                                   \
    if (_dev_guard.err != hipSuccess) return fail(MCBS_EHIP, "cannot select device %d: %s", (b)->cfg.device, hipGetErrorString(_dev_guard.err))

static FastDiv fast_div_host(uint32_t d) {   // n / d = (t + ((n - t) >> sh1)) >> sh2 with t = mulhi(n, mul)
    uint32_t l = 0;
    while ((1ull << l) < d) ++l;
    FastDiv f;
    f.mul = (uint32_t)(((1ull << 32) * ((1ull << l) - d)) / d + 1ull);
    f.sh1 = l < 1u ? l : 1u;
    f.sh2 = l > 0u ? l - 1u : 0u;
    return f;
}

// "No array this call writes may share a byte with another array it reads or writes" (mcbs_extents.h), as every entry point refuses it
static int disjoint(const char* who, const Extents& x) {
    if (x.overflowed) return fail(MCBS_ELIMIT, "%s: more than %zu arrays in one overlap check", who, Extents::kCapacity);
    const Extents::Pair c = x.overlap();
    if (c.first) return fail(MCBS_EINVAL, "%s: %s%s overlaps %s%s", who, c.first->prefix, c.first->name, c.second->prefix, c.second->name);
    return MCBS_OK;
}

// The arrays of a buffer struct of mcbs.h, one entry per pointer member in the member's order: n_envs rows of
// bytes + per_node * n_nodes + per_service * n_services bytes each; all three 0: the member is in no overlap check.
// kind kFreshRow: ONE such row for the whole batch, which the call only ever reads, whatever the struct's other arrays are listed as
enum ArrayKind : uint32_t { kPerEnv = 0, kFreshRow = 1 };
struct ArrayDesc { const char* name; uint32_t bytes, per_node, per_service; ArrayKind kind; };
static const ArrayDesc kWrapperArrays[] = {
    {"invalid", 1}, {"reward", 4}, {"terminated", 1}, {"timesteps", 4}, {"valid_action_count", 8}, {"invalid_action_count", 8}, {"episode_returns", 8},
    {"last_cyber_reward", 4}, {"has_cyber_reward", 1}, {"rewards", 4}, {"truncated", 1}, {"dones", 1}, {"episode_return_out", 8},
    {"episode_length_out", 4}, {"n_done", 0}, {"executed", 1}};
static const ArrayDesc kInfoArrays[] = {{"network_availability", 8}, {"step_count", 4}, {"truncated", 1}, {"out_of_bound", 1}, {"raw_reward", 4}};
static const ArrayDesc kDefenderObsArrays[] = {
    {"infected_nodes", 0, 1}, {"incoming_firewall_status", 0, 6}, {"outgoing_firewall_status", 0, 6}, {"services_status", 0, 0, 1}};
// (dw->attacker_has_cyber_reward / attacker_last_cyber_reward ARE w->has_cyber_reward / last_cyber_reward: read where the attacker half wrote)
static const ArrayDesc kDefenderWrapperArrays[] = {
    {"valid", 1}, {"availability", 8}, {"evicted", 1}, {"attacker_has_cyber_reward", 0}, {"attacker_last_cyber_reward", 0}, {"timesteps", 4},
    {"valid_action_count", 8}, {"invalid_action_count", 8}, {"has_breached_sla", 1}, {"prev_availability", 8}, {"reward", 8}, {"terminated", 1},
    {"truncated", 1}, {"breached", 1}, {"won", 1}};
static const ArrayDesc kTrainingArrays[] = {
    {"attacker_reset_request", 1}, {"defender_return", 8}, {"attacker_valid_out", 8}, {"attacker_invalid_out", 8}, {"defender_return_out", 8},
    {"defender_length_out", 4}, {"defender_valid_out", 8}, {"defender_invalid_out", 8}, {"defender_dones", 1}, {"terminal_infected_nodes", 0, 1},
    {"terminal_incoming_firewall_status", 0, 6}, {"terminal_outgoing_firewall_status", 0, 6}, {"terminal_services_status", 0, 0, 1},
    {"fresh_infected_nodes", 0, 1, 0, kFreshRow}, {"fresh_incoming_firewall_status", 0, 6, 0, kFreshRow},
    {"fresh_outgoing_firewall_status", 0, 6, 0, kFreshRow},
    {"fresh_services_status", 0}};
// (the two packed members are rows of the caller's stride: mcbs_two_agent_train_step_packed lists them itself)
static const ArrayDesc kTrainingPackedArrays[] = {
    {"attacker_reset_request", 1}, {"defender_return", 8}, {"attacker_valid_out", 8}, {"attacker_invalid_out", 8}, {"defender_return_out", 8},
    {"defender_length_out", 4}, {"defender_valid_out", 8}, {"defender_invalid_out", 8}, {"defender_dones", 1}, {"terminal_defender_packed", 0},
    {"fresh_defender_packed", 0}};
// ... appended to an overlap check as prefix + name
template <class W, size_t K>
static void add_arrays(Extents& x, const char* prefix, const W* w, const ArrayDesc (&desc)[K], uint64_t E, uint64_t N, uint64_t Sv, bool written) {
    // (the count is held to the header here; the ORDER only by tests/test_gpu_turn_extents.py, which moves an array of every struct)
    static_assert(sizeof(W) == K * sizeof(void*), "one descriptor per pointer member of the struct (mcbs.h)");
    const void* const* p = reinterpret_cast<const void* const*>(w);
    for (size_t i = 0; w && i < K; ++i) {
        const bool fresh_row = desc[i].kind == kFreshRow;
        x.bytes(desc[i].name, p[i], (fresh_row ? 1u : E) * (desc[i].bytes + desc[i].per_node * N + desc[i].per_service * Sv), written && !fresh_row, prefix);
    }
}

struct HotLayout {
    uint32_t node, desc, payload, auth, auth_words, triple, avail, fwlist, bytes;
    uint32_t max_leak;   // the largest payload_cnt of any descriptor: no action of this topology leaks more entries (StepCfg::max_leak)
    uint32_t traits;     // MCBS_TOPO_* (mcbs.h): what the descriptors and the node count make possible; the narrow lean step is chosen by them
};

struct mcbs_topology {
    std::vector<uint8_t> host;
    std::vector<uint8_t> hot_host;  // step kernel's view of the tables (mcbs_device.h "hot image")
    HotLayout hot{};
    uint8_t* dev = nullptr;
    uint8_t* hot_dev = nullptr;
    int32_t device = 0;
    const mcbs_topo_header* H() const { return reinterpret_cast<const mcbs_topo_header*>(host.data()); }
};

struct mcbs_batch {
    const mcbs_topology* topo = nullptr;
    mcbs_batch_cfg cfg{};
    DevState S{};
    Topo T{};
    StepCfg C{};
    StepCfg* C_dev = nullptr;       // device copy read by the step kernel through the scalar cache
    uint32_t* ere_lists_dev = nullptr;
    DefPackGeom def_pack{};         // MCBS_DEFENDER_EXTERNAL: the packed defender observation's geometry; .svc = the services' bits of a row (device)
    // developer switches, read ONCE at batch creation (getenv on every launch costs more than the launch itself)
    bool no_fused_masks = false, slow_masks = false, no_row_masks = false;
    bool no_quad_obs = false;       // MCBS_NO_QUAD_OBS=1: a wavefront per env for small topologies' observations with mask fields (rounds 1-2)
    bool force_quad_obs = false;    // MCBS_QUAD_OBS=1: obs_quad_kernel also where mask rows are whole cache lines
    bool no_block_masks = false;    // MCBS_NO_BLOCK_MASKS=1: round 2's fused mask writers (rows switched on / off per chunk)
    size_t disc_stride = 0;         // mcbs_set_mask_discrete_stride: bytes between two envs' rows of mask_discrete (0: dense)
    mcbs_batch_variant_info variant{};   // which kernels the batch's calls dispatch to: decided once, by batch_variant at the end of mcbs_batch_create
    bool lean_step = false;         // mcbs_step without info buffers takes the lean argument block (packed, no defender, reset image in the
                                    // config); decided once, in mcbs_batch_create
    bool narrow_step = false;       // ... and the narrow instantiation of that kernel: the topology has no trait beyond kNarrowStepCan
                                    // (mcbs_step.hip); decided once, in mcbs_batch_create
    uint8_t* arena = nullptr;       // every per-env column + bodies + init body, one allocation
    size_t arena_bytes = 0;
    ObsDigest* digest = nullptr;
    ObsDigest* reset_digest = nullptr;   // the digest of a freshly reset env, captured by the first observation after a whole-batch reset
    bool all_fresh = true, reset_digest_ok = false;
    // what mcbs_mask_logits may trust: 0 = no observation has written the per-env digests since the batch was created / wholly reset /
    // given a state (mcbs_set_state); 1 = every env's digest is the one its last observation wrote; 2 = some envs were reset by mask
    // since (their digests are stale until mcbs_observe_masked has re-observed them)
    int digest_state = 0;
    bool digest_lists = false;           // some digests may carry the discovery order of their own observation (ObsDigest::pad: the two-agent training
                                         // turn wrote them): the kernels that rebuild the mask from the digest run their OWN instantiations
    const double* tape = nullptr;
    uint32_t tape_dps = 0;
    unsigned long long* stamps = nullptr;   // diagnostic builds: device buffer [waves][8]
    // timing
    bool timing = false;
    std::vector<hipEvent_t> ev;     // pairs (start, stop) per launch
    size_t ev_used = 0;
    double timed_ms = 0.0;
    uint64_t timed_launches = 0;
};

extern "C" const char* mcbs_last_error(void) { return g_err; }
extern "C" uint32_t mcbs_abi_version(void) { return MCBS_ABI_VERSION; }

// ------------------------------------------------------------------ topology
static int check_section(const mcbs_topo_header* h, uint32_t off, size_t bytes, const char* name) {
    if (off % 16u || (size_t)off + bytes > h->total_bytes) return fail(MCBS_EINVAL, "topology blob: section %s out of range", name);
    return MCBS_OK;
}

// Everything mcbs_topology_create checks about a blob before it builds anything from it (host only)
static int check_blob(const void* blob, size_t nbytes) {
    if (nbytes < sizeof(mcbs_topo_header)) return fail(MCBS_EINVAL, "topology blob too small");
    const mcbs_topo_header* h = static_cast<const mcbs_topo_header*>(blob);
    if (h->magic != MCBS_TOPO_MAGIC) return fail(MCBS_EINVAL, "topology blob: bad magic");
    if (h->abi_version != MCBS_ABI_VERSION) return fail(MCBS_EINVAL, "topology blob: ABI version %u, library %u", h->abi_version, MCBS_ABI_VERSION);
    if (h->total_bytes != nbytes || h->header_bytes != sizeof(mcbs_topo_header)) return fail(MCBS_EINVAL, "topology blob: size mismatch");
    if (h->n_nodes == 0 || h->n_nodes > MCBS_MAX_NODES) return fail(MCBS_ELIMIT, "n_nodes %u outside 1..%d", h->n_nodes, MCBS_MAX_NODES);
    if (h->n_ports == 0 || h->n_ports > MCBS_MAX_PORTS || h->n_props > 60u || h->max_slots == 0 || h->max_slots > MCBS_MAX_SLOTS ||
        h->n_local == 0 || h->n_local > MCBS_MAX_LOCAL_VULNS || h->n_remote == 0 || h->n_local + h->n_remote > MCBS_MAX_VULN_COLUMNS ||
        h->n_cred_strings > MCBS_MAX_CRED_STRINGS ||
        h->n_triples > MCBS_MAX_TRIPLES)
        return fail(MCBS_ELIMIT, "topology exceeds an engine limit");
    int rc;
    if ((rc = check_section(h, h->off_node, sizeof(mcbs_node_static) * h->n_nodes, "node"))) return rc;
    if ((rc = check_section(h, h->off_slot_of, (size_t)h->n_nodes * (h->n_local + h->n_remote), "slot_of"))) return rc;
    if ((rc = check_section(h, h->off_slot, sizeof(mcbs_vuln_slot) * h->n_nodes * h->max_slots, "slot"))) return rc;
    if ((rc = check_section(h, h->off_payload, sizeof(mcbs_payload) * h->n_payload, "payload"))) return rc;
    if ((rc = check_section(h, h->off_service, sizeof(mcbs_service) * h->n_services, "service"))) return rc;
    if ((rc = check_section(h, h->off_allowed, sizeof(uint16_t) * h->n_allowed, "allowed"))) return rc;
    if ((rc = check_section(h, h->off_triple, sizeof(mcbs_triple) * h->n_triples, "triple"))) return rc;
    if ((rc = check_section(h, h->off_init_order, h->n_nodes, "init_order"))) return rc;
    // every index the kernels will dereference is range-checked here, once, on the host
    const uint8_t* b = static_cast<const uint8_t*>(blob);
    const mcbs_node_static* ns = reinterpret_cast<const mcbs_node_static*>(b + h->off_node);
    const mcbs_vuln_slot* sl = reinterpret_cast<const mcbs_vuln_slot*>(b + h->off_slot);
    const mcbs_payload* pl = reinterpret_cast<const mcbs_payload*>(b + h->off_payload);
    const mcbs_service* sv = reinterpret_cast<const mcbs_service*>(b + h->off_service);
    const uint8_t* so = b + h->off_slot_of;
    for (uint32_t n = 0; n < h->n_nodes; ++n) {
        if ((uint32_t)ns[n].svc_off + ns[n].svc_cnt > h->n_services) return fail(MCBS_EINVAL, "node %u: service range", n);
        if (ns[n].n_slots > h->max_slots) return fail(MCBS_EINVAL, "node %u: slot count", n);
        for (uint32_t c = 0; c < h->n_local + h->n_remote; ++c) {
            const uint8_t s = so[(size_t)n * (h->n_local + h->n_remote) + c];
            if (s != 0xFF && s >= ns[n].n_slots) return fail(MCBS_EINVAL, "node %u: slot_of out of range", n);
        }
        for (uint32_t s = 0; s < ns[n].n_slots; ++s) {
            const mcbs_vuln_slot& v = sl[(size_t)n * h->max_slots + s];
            if ((size_t)v.payload_off + v.payload_cnt > h->n_payload) return fail(MCBS_EINVAL, "node %u slot %u: payload range", n, s);
            if (v.level > 3 || v.kind > MCBS_OUT_OTHER) return fail(MCBS_EINVAL, "node %u slot %u: bad kind/level", n, s);
            if (v.payload_cnt > 1023) return fail(MCBS_ELIMIT, "node %u slot %u: payload too long", n, s);
        }
    }
    for (uint32_t i = 0; i < h->n_payload; ++i)
        if (pl[i].node >= h->n_nodes || (h->n_cred_strings && pl[i].cred >= h->n_cred_strings && pl[i].cred != 0) ||
            (h->n_triples && pl[i].triple >= h->n_triples && pl[i].triple != 0) || pl[i].port >= h->n_ports)
            return fail(MCBS_EINVAL, "payload %u out of range", i);
    for (uint32_t i = 0; i < h->n_services; ++i)
        if ((uint32_t)sv[i].allowed_off + sv[i].allowed_cnt > h->n_allowed || sv[i].port >= h->n_ports)
            return fail(MCBS_EINVAL, "service %u out of range", i);
    const mcbs_triple* tr = reinterpret_cast<const mcbs_triple*>(b + h->off_triple);
    for (uint32_t i = 0; i < h->n_triples; ++i)
        if (tr[i].node >= h->n_nodes || tr[i].cred >= h->n_cred_strings || tr[i].port >= h->n_ports)
            return fail(MCBS_EINVAL, "triple %u out of range", i);
    if ((rc = check_section(h, h->off_fw_list0, 2u * (size_t)h->n_fw_lists, "fw_list0"))) return rc;
    if ((rc = check_section(h, h->off_fw_range, 2u * sizeof(uint16_t) * (size_t)h->n_fw_lists, "fw_range"))) return rc;
    if ((rc = check_section(h, h->off_fw_rule, sizeof(mcbs_fw_rule) * (size_t)h->n_fw_rules, "fw_rule"))) return rc;
    if (h->n_names > 256u) return fail(MCBS_ELIMIT, "more than 256 firewall port names");
    {   // every rule list lies inside the rule array and every rule names a known port (mcbs_batch_create and the random-events
        // kernels index with these)
        const uint16_t* fr = reinterpret_cast<const uint16_t*>(b + h->off_fw_range);
        const mcbs_fw_rule* fwr = reinterpret_cast<const mcbs_fw_rule*>(b + h->off_fw_rule);
        for (uint32_t l = 0; l < h->n_fw_lists; ++l)
            if ((uint32_t)fr[2 * l] + fr[2 * l + 1] > h->n_fw_rules) return fail(MCBS_EINVAL, "firewall rule list %u out of range", l);
        for (uint32_t i = 0; i < h->n_fw_rules; ++i)
            if (fwr[i].name >= h->n_names) return fail(MCBS_EINVAL, "firewall rule %u: port name out of range", i);
        for (int i = 0; i < 6; ++i)
            if (h->rule_port[i] != 0xFFu && h->rule_port[i] >= h->n_ports) return fail(MCBS_EINVAL, "rule_port[%d] out of range", i);
    }
    for (uint32_t n = 0; n < h->n_nodes; ++n)
        if ((ns[n].fw_lists & 0xFFFFu) >= h->n_fw_lists || (ns[n].fw_lists >> 16) >= h->n_fw_lists) return fail(MCBS_EINVAL, "node %u: firewall list id", n);
    if (h->off_ere) {          // ExternalRandomEvents tables: every index a kernel will use as a bit position or an array subscript
        if ((rc = check_section(h, h->off_ere, sizeof(mcbs_ere_tables), "ere"))) return rc;
        const mcbs_ere_tables* et = reinterpret_cast<const mcbs_ere_tables*>(b + h->off_ere);
        const uint32_t W = h->n_local + h->n_remote;
        const size_t room = h->total_bytes - h->off_ere;
        if (W > 64u || et->n_library > W || et->key_cap == 0 || et->key_cap > 255u ||
            (size_t)et->off_own_keys + (size_t)et->key_cap * h->n_nodes > room || (size_t)et->off_own_cnt + h->n_nodes > room ||
            (size_t)et->off_lib_sorted + et->n_library > room)
            return fail(MCBS_EINVAL, "topology blob: random-events tables out of range");
        const uint8_t* eb = reinterpret_cast<const uint8_t*>(et);
        for (uint32_t n = 0; n < h->n_nodes; ++n) {
            const uint32_t cnt = eb[et->off_own_cnt + n];
            if (cnt + et->n_library > et->key_cap) return fail(MCBS_EINVAL, "node %u: vulnerability key list longer than its capacity", n);
            for (uint32_t k = 0; k < cnt; ++k)
                if (eb[et->off_own_keys + (size_t)n * et->key_cap + k] >= W) return fail(MCBS_EINVAL, "node %u: vulnerability key out of range", n);
        }
        for (uint32_t i = 0; i < et->n_library; ++i) if (eb[et->off_lib_sorted + i] >= W) return fail(MCBS_EINVAL, "library column out of range");
        for (int i = 0; i < 7; ++i) if (et->sample_name[i] >= h->n_names) return fail(MCBS_EINVAL, "sample port name out of range");
        if (W < 64u && (et->lib_cols >> W)) return fail(MCBS_EINVAL, "library column mask out of range");
    }
    const uint8_t* io = b + h->off_init_order;
    if (h->n_init_owned > h->n_nodes) return fail(MCBS_EINVAL, "init order");
    for (uint32_t i = 0; i < h->n_init_owned; ++i) if (io[i] >= h->n_nodes) return fail(MCBS_EINVAL, "init order");
    return MCBS_OK;
}

// The topology's traits (MCBS_TOPO_*, mcbs.h) from a checked blob: one pass over the vulnerability slots that some column reaches — the
// descriptors of the hot image, the only ones an action can name — and the node count
static uint32_t topo_traits(const void* blob) {
    const uint8_t* b = static_cast<const uint8_t*>(blob);
    const mcbs_topo_header* h = static_cast<const mcbs_topo_header*>(blob);
    const mcbs_vuln_slot* sl = reinterpret_cast<const mcbs_vuln_slot*>(b + h->off_slot);
    const uint8_t* so = b + h->off_slot_of;
    const uint32_t W = h->n_local + h->n_remote;
    uint32_t t = h->n_nodes > 12u ? MCBS_TOPO_WIDE_ROWS : 0u;
    for (uint32_t n = 0; n < h->n_nodes; ++n)
        for (uint32_t c = 0; c < W; ++c) {
            const uint8_t s = so[(size_t)n * W + c];
            if (s == 0xFF) continue;
            const mcbs_vuln_slot& v = sl[(size_t)n * h->max_slots + s];
            if (v.kind == MCBS_OUT_PRIVILEGE_ESCALATION) t |= MCBS_TOPO_ESCALATION;
            if (v.kind == MCBS_OUT_LATERAL_MOVE) t |= MCBS_TOPO_LATERAL_EXPLOIT;
            if (v.kind == MCBS_OUT_PROBE_SUCCEEDED) t |= MCBS_TOPO_PROBE;
            if (v.precond_tt != 0xFFFFu) t |= MCBS_TOPO_PRECONDITION;
            if (v.payload_cnt > 1u) t |= MCBS_TOPO_MULTI_LEAK;
        }
    return t;
}

extern "C" int mcbs_topology_traits(const void* blob, size_t nbytes, uint32_t* traits) {
    if (!blob || !traits) return fail(MCBS_EINVAL, "null argument");
    if (const int rc = check_blob(blob, nbytes)) return rc;
    *traits = topo_traits(blob);
    return MCBS_OK;
}

extern "C" int mcbs_topology_create(const void* blob, size_t nbytes, int32_t device, mcbs_topology** out) {
    if (!blob || !out) return fail(MCBS_EINVAL, "null argument");
    if (const int rc = check_blob(blob, nbytes)) return rc;
    const uint8_t* b = static_cast<const uint8_t*>(blob);
    const mcbs_topo_header* h = static_cast<const mcbs_topo_header*>(blob);
    const mcbs_node_static* ns = reinterpret_cast<const mcbs_node_static*>(b + h->off_node);
    const mcbs_vuln_slot* sl = reinterpret_cast<const mcbs_vuln_slot*>(b + h->off_slot);
    const mcbs_payload* pl = reinterpret_cast<const mcbs_payload*>(b + h->off_payload);
    const mcbs_service* sv = reinterpret_cast<const mcbs_service*>(b + h->off_service);
    const uint8_t* so = b + h->off_slot_of;
    const mcbs_triple* tr = reinterpret_cast<const mcbs_triple*>(b + h->off_triple);

    mcbs_topology* t = new (std::nothrow) mcbs_topology();
    if (!t) return fail(MCBS_ENOMEM, "out of memory");
    t->host.assign(b, b + nbytes);
    t->device = device;
    {   // hot image: 32-byte node records, flattened (node, column) descriptors, then the list sections verbatim
        const uint32_t N = h->n_nodes, W = h->n_local + h->n_remote;
        HotLayout& L = t->hot;
        L.traits = topo_traits(blob);
        uint32_t off = 0;
        auto take = [&](size_t bytes) { uint32_t o = off; off = (uint32_t)((off + bytes + 15) / 16 * 16); return o; };
        L.node = take(sizeof(HotNode) * N);
        // every section holds at least one (zero) record: the step kernel looks tables up with clamped indices for every lane
        L.desc = take(sizeof(HotDesc) * ((size_t)N * W + 1));
        L.payload = take(sizeof(mcbs_payload) * (h->n_payload + 1));
        // authorisation table replacing the service / allowed-credential lists (actions.py:608-621): per (node, port) the set
        // of credential strings that some RUNNING service on that port accepts (service state never changes, mcbs_defend.hip)
        // ... indexed by the TRIPLE id of the cached credential the action names (bit t: the credential string of triple t is accepted),
        // so that the look-up does not wait for the triple -> credential-string load
        const uint32_t P1 = h->n_ports ? h->n_ports : 1u;
        L.auth_words = (h->n_triples + 63u) / 64u ? (h->n_triples + 63u) / 64u : 1u;
        L.auth = take(sizeof(uint64_t) * (size_t)N * P1 * L.auth_words);
        L.triple = take(sizeof(mcbs_triple) * (h->n_triples + 1));
        L.avail = take(sizeof(double) * N);
        L.fwlist = take(sizeof(uint32_t) * N);
        L.bytes = off;
        t->hot_host.assign(off, 0);
        uint8_t* hb = t->hot_host.data();
        for (uint32_t n = 0; n < N; ++n) {
            HotNode hn{};
            hn.props = ns[n].props; hn.value = ns[n].value; hn.fw_in_allow = ns[n].fw_in_allow; hn.fw_out_allow = ns[n].fw_out_allow;
            hn.listen = ns[n].listen; hn.svc_off = ns[n].svc_off; hn.svc_cnt = ns[n].svc_cnt; hn.flags = ns[n].flags;
            memcpy(hb + L.node + sizeof(HotNode) * n, &hn, sizeof(hn));
            memcpy(hb + L.avail + sizeof(double) * n, &ns[n].avail_term, sizeof(double));
            memcpy(hb + L.fwlist + sizeof(uint32_t) * n, &ns[n].fw_lists, sizeof(uint32_t));
            for (uint32_t c = 0; c < W; ++c) {
                HotDesc d{};
                const uint8_t s = so[(size_t)n * W + c];
                d.kind = 0xFF;
                if (s != 0xFF) {
                    const mcbs_vuln_slot& v = sl[(size_t)n * h->max_slots + s];
                    d.cost = v.cost; d.probe_mask = v.probe_mask; d.payload_off = v.payload_off; d.payload_cnt = v.payload_cnt;
                    d.precond_tt = v.precond_tt; d.kind = v.kind; d.level = v.level; d.slot = s;
                    for (uint32_t i = 0; i < 4u && i < v.payload_cnt; ++i) d.inline_payload[i] = pl[v.payload_off + i];
                    if (v.payload_cnt > L.max_leak) L.max_leak = v.payload_cnt;
                }
                memcpy(hb + L.desc + sizeof(HotDesc) * ((size_t)n * W + c), &d, sizeof(d));
            }
        }
        memcpy(hb + L.payload, pl, sizeof(mcbs_payload) * h->n_payload);
        const uint16_t* allowed = reinterpret_cast<const uint16_t*>(b + h->off_allowed);
        uint64_t* auth = reinterpret_cast<uint64_t*>(hb + L.auth);
        for (uint32_t n = 0; n < N; ++n)
            for (uint32_t i = ns[n].svc_off; i < (uint32_t)ns[n].svc_off + ns[n].svc_cnt; ++i) {
                if (!sv[i].running) continue;
                for (uint32_t k = 0; k < sv[i].allowed_cnt; ++k) {
                    const uint32_t c = allowed[sv[i].allowed_off + k];
                    for (uint32_t t3 = 0; t3 < h->n_triples; ++t3)         // every cached credential that carries this string
                        if (tr[t3].cred == c) auth[((size_t)n * P1 + sv[i].port) * L.auth_words + (t3 >> 6)] |= 1ull << (t3 & 63u);
                }
            }
        memcpy(hb + L.triple, tr, sizeof(mcbs_triple) * h->n_triples);
    }
    DeviceGuard guard(device);
    hipError_t e = guard.err;
    if (e == hipSuccess) e = hipMalloc(&t->dev, nbytes);
    if (e == hipSuccess) e = hipMemcpy(t->dev, blob, nbytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(&t->hot_dev, t->hot_host.size());
    if (e == hipSuccess) e = hipMemcpy(t->hot_dev, t->hot_host.data(), t->hot_host.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (t->dev) (void)hipFree(t->dev);
        if (t->hot_dev) (void)hipFree(t->hot_dev);
        delete t;
        return fail(MCBS_EHIP, "topology upload failed: %s", hipGetErrorString(e));
    }
    *out = t;
    return MCBS_OK;
}

extern "C" void mcbs_topology_destroy(mcbs_topology* t) {
    if (!t) return;
    DeviceGuard guard(t->device);
    if (t->dev) (void)hipFree(t->dev);
    if (t->hot_dev) (void)hipFree(t->hot_dev);
    delete t;
}

// ------------------------------------------------------------------ batch
static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// reset_kernel: the envs env_mask names (NULL: all) back to step zero of a fresh episode; next_episode 1: as a new episode (mcbs_reset),
// 0: the batch as it was created (mcbs_rewind)
static void launch_step_zero(mcbs_batch* b, const uint8_t* env_mask, int next_episode, hipStream_t st) {
    hipLaunchKernelGGL(reset_kernel, dim3((b->S.E + 127) / 128), dim3(128), 0, st, b->S, b->T, env_mask, next_episode);
}

// Which compiled variant the batch's calls dispatch to (mcbs_batch_variant_info, mcbs.h): everything it depends on is fixed once
// mcbs_batch_create has laid the batch out, so it is decided there, once, and the launches read b->variant.
static mcbs_batch_variant_info batch_variant(const mcbs_batch* b) {
    const DevState& S = b->S;
    const uint32_t def = b->cfg.defender_kind;
    mcbs_batch_variant_info v{};
    v.packed = S.packed; v.words_per_set = S.WT; v.wide = S.wide; v.defender_kind = def;
    // large topologies: G = WT lanes per env (mcbs_step_coop.hip).  More than 64 nodes guarantees the list regions its level-1 loads
    // cover (16 G discovery-order bytes, 32 G credential-cache bytes) lie inside the env's body; MCBS_NO_COOP=1: the one-lane kernel
    // It pays while the one-lane kernel would leave SIMDs idle: measured on MI355X (profiles/round3_notes.md) 4.43 vs 4.96 us for
    // 8 192 Chain-100 envs and 6.0 vs 7.4 us for 16 384 Random-256 envs, but 9.2 vs 9.0 us at 65 536 and 24.7 vs 22.9 us at 131 072 envs
    // (the chip is full either way and the G lanes' redundant scalar work then costs issue slots): up to 512 one-lane wavefronts.
    uint32_t coop_max_envs = 32768u;
    if (const char* ov = getenv("MCBS_COOP_MAX_ENVS")) coop_max_envs = (uint32_t)strtoul(ov, nullptr, 10);   // experiments
    v.coop = !S.packed && S.WT >= 2u && S.N > 64u && !S.wide && !getenv("MCBS_NO_COOP") && S.E <= coop_max_envs &&
             (def == MCBS_DEFENDER_NONE || def == MCBS_DEFENDER_SCAN_AND_REIMAGE);
    // mcbs_attacker_wrapper_step in ONE launch (mcbs_wrapper_fused.hip): packed batch whose reset image is held in the config, at most 16
    // nodes / cached credentials; MCBS_NO_FUSED_WRAPPER=1 keeps the three launches (tests step both)
    v.fused_wrapper = !(getenv("MCBS_NO_FUSED_WRAPPER") || b->no_fused_masks || !S.packed || !b->C.init_image_ok || S.N > 16u ||
                        b->cfg.maximum_node_count > 16u || b->cfg.maximum_total_credentials > 16u || b->topo->H()->n_triples > 15u ||
                        def == MCBS_DEFENDER_RANDOM_EVENTS);
    // the learned defender's observation written by the turn kernel's own workgroups (one launch per turn): topologies of up to 32 nodes
    // and 256 services; MCBS_NO_FUSED_DEFENDER_OBS=1: the separate launch
    v.fused_defender_obs = def == MCBS_DEFENDER_EXTERNAL && S.N <= 32u && b->C.n_services <= 256u && !getenv("MCBS_NO_FUSED_DEFENDER_OBS");
    return v;
}

extern "C" int mcbs_batch_variant(const mcbs_batch* b, mcbs_batch_variant_info* out) {
    if (!b || !out) return fail(MCBS_EINVAL, "null argument");
    *out = b->variant;
    return MCBS_OK;
}

extern "C" int32_t mcbs_step_is_lean(const mcbs_batch* b, int32_t with_info) {
    return (b && b->lean_step && !with_info) ? 1 : 0;
}
extern "C" int32_t mcbs_step_topo_traits(const mcbs_batch* b, int32_t with_info, uint32_t* traits) {
    if (traits) *traits = b ? b->topo->hot.traits : 0u;
    return (b && b->narrow_step && !with_info) ? 1 : 0;
}

extern "C" int mcbs_batch_create(const mcbs_topology* topo, const mcbs_batch_cfg* cfg, mcbs_batch** out) {
    if (!topo || !cfg || !out) return fail(MCBS_EINVAL, "null argument");
    if (cfg->abi_version != MCBS_ABI_VERSION) return fail(MCBS_EINVAL, "cfg ABI version %u, library %u", cfg->abi_version, MCBS_ABI_VERSION);
    const mcbs_topo_header* h = topo->H();
    if (cfg->n_envs == 0) return fail(MCBS_EINVAL, "n_envs must be positive");
    if (cfg->device != topo->device) return fail(MCBS_EINVAL, "batch and topology are on different devices");
    // CyberBattleEnv.validate_environment (cyberbattle_env.py:416-435)
    if (h->n_nodes > cfg->maximum_node_count)
        return fail(MCBS_EINVAL, "Network node count (%u) exceeds the specified limit of %u.", h->n_nodes, cfg->maximum_node_count);
    if (cfg->maximum_node_count > MCBS_MAX_NODES) return fail(MCBS_ELIMIT, "maximum_node_count %u > %d", cfg->maximum_node_count, MCBS_MAX_NODES);
    if (h->max_leak_per_action > cfg->maximum_discoverable_credentials_per_action)
        return fail(MCBS_EINVAL, "Some action in the environment returns %u credentials which exceeds the maximum number of discoverable credentials of %u",
                    h->max_leak_per_action, cfg->maximum_discoverable_credentials_per_action);
    if (cfg->maximum_total_credentials == 0 || cfg->maximum_total_credentials > 65535u) return fail(MCBS_ELIMIT, "maximum_total_credentials out of range");
    if (h->n_triples > cfg->maximum_total_credentials)
        return fail(MCBS_ELIMIT, "the topology can leak %u distinct credentials but maximum_total_credentials is %u "
                    "(the reference would overflow its observation space)", h->n_triples, cfg->maximum_total_credentials);
    if (cfg->maximum_discoverable_credentials_per_action > 1023u) return fail(MCBS_ELIMIT, "maximum_discoverable_credentials_per_action too large");
    if (cfg->defender_kind > MCBS_DEFENDER_RANDOM_EVENTS) return fail(MCBS_EINVAL, "unknown defender kind");
    const bool random_events = cfg->defender_kind == MCBS_DEFENDER_RANDOM_EVENTS;
    if (random_events && !h->off_ere) return fail(MCBS_EINVAL, "the topology blob carries no ExternalRandomEvents tables (off_ere)");
    if (cfg->defender_kind == MCBS_DEFENDER_SCAN_AND_REIMAGE && cfg->scan_frequency == 0) return fail(MCBS_EINVAL, "scan_frequency must be positive");
    if (cfg->rng_kind > MCBS_RNG_TAPE) return fail(MCBS_EINVAL, "unknown rng kind");
    if (h->n_cred_strings > MCBS_MAX_CRED_STRINGS || h->n_triples > MCBS_MAX_TRIPLES)
        return fail(MCBS_ELIMIT, "at most %d credential strings / %d triples (topology has %u / %u)", MCBS_MAX_CRED_STRINGS, MCBS_MAX_TRIPLES,
                    h->n_cred_strings, h->n_triples);

    mcbs_batch* b = new (std::nothrow) mcbs_batch();
    if (!b) return fail(MCBS_ENOMEM, "out of memory");
    b->topo = topo;
    b->cfg = *cfg;
    b->no_fused_masks = getenv("MCBS_NO_FUSED_MASKS") != nullptr;
    b->slow_masks = getenv("MCBS_SLOW_MASKS") != nullptr; b->no_row_masks = getenv("MCBS_NO_ROW_MASKS") != nullptr;
    b->no_block_masks = getenv("MCBS_NO_BLOCK_MASKS") != nullptr;
    b->no_quad_obs = getenv("MCBS_NO_QUAD_OBS") != nullptr; b->force_quad_obs = getenv("MCBS_QUAD_OBS") != nullptr;
    const uint32_t E = cfg->n_envs, N = h->n_nodes;
    DevState& S = b->S;
    S.E = E; S.N = N; S.NW = (N + 63) / 64;
    S.SW = (h->n_cred_strings + 63) / 64; if (!S.SW) S.SW = 1;
    S.TW = (h->n_triples + 63) / 64; if (!S.TW) S.TW = 1;
    S.Cmax = cfg->maximum_total_credentials;
    S.off_disc = 0;                                                             // u8 discovery order, >= 16 bytes
    // both lists have one slack entry past their capacity: the cooperative step kernel (mcbs_step_coop.hip) and the looping variant of
    // mcbs_step.hip (mcbs_step_many / mcbs_rollout_random) append every leaked element and only advance the count for a new one; the
    // other step kernels store new elements only
    S.off_cred = (uint32_t)align_up((size_t)N + 1, 16);                         // u16 credential cache, >= 32 bytes
    S.off_rows = (uint32_t)align_up((size_t)S.off_cred + (2u * (h->n_triples + 1u) > 32u ? 2u * (h->n_triples + 1u) : 32u), 16);
    const bool external = cfg->defender_kind == MCBS_DEFENDER_EXTERNAL;
    // small topologies (Chain-10, ToyCtf): the eight sets of an env as 16-bit fields of one 16-byte word and 4-byte node rows,
    // so that the header and the WHOLE body are level-1 loads (mcbs_device.h); node and triple ids fit a nibble, so both lists
    // (at most 16 nodes, fewer than 16 triples) are one more 16-byte word behind the sets, and the body is rows only
    S.tiny_p = h->n_props; S.tiny_v = h->max_slots;
    S.packed = (N <= 16u && h->n_cred_strings <= 16u && h->n_triples < 16u && S.tiny_p + 4u + 2u * S.tiny_v <= 32u &&
                !getenv("MCBS_NO_PACKED_SETS")) ? 1u : 0u;
    if (S.packed) S.off_disc = S.off_cred = S.off_rows = 0u;
    const size_t row_bytes = S.packed ? 4u : sizeof(Row);
    S.off_fw = external ? (uint32_t)align_up((size_t)S.off_rows + row_bytes * N, 16) : 0u;
    size_t body_end = external ? (size_t)S.off_fw + 2u * h->n_fw_lists : (size_t)S.off_rows + row_bytes * N;
    // ExternalRandomEvents overlay (mcbs_ere.hip): key lists, key counts, presence masks, service bits, rule lists {count, entries}
    StepCfg& C0 = b->C;
    std::vector<uint32_t> ere_lists;
    if (random_events) {
        const mcbs_ere_tables* et = reinterpret_cast<const mcbs_ere_tables*>(topo->host.data() + h->off_ere);
        C0.ere_key_cap = et->key_cap; C0.ere_n_library = et->n_library; C0.ere_lib_cols = et->lib_cols; C0.off_ere = h->off_ere;
        C0.ere_off_present = (uint32_t)align_up(body_end, 8);
        C0.ere_off_svc = C0.ere_off_present + 8u * N;
        C0.ere_off_keys = C0.ere_off_svc + 4u * N;
        C0.ere_off_kcnt = C0.ere_off_keys + et->key_cap * N;
        C0.ere_off_fw = (uint32_t)align_up((size_t)C0.ere_off_kcnt + N, 2);
        const uint16_t* fr = reinterpret_cast<const uint16_t*>(topo->host.data() + h->off_fw_range);
        uint32_t off = 0;
        for (uint32_t l = 0; l < h->n_fw_lists; ++l) {
            const uint32_t cap = fr[l * 2 + 1] + MCBS_FW_GROWTH;
            if (off > 0xFFFFu) { delete b; return fail(MCBS_ELIMIT, "firewall rule lists too large for the random-events overlay"); }
            ere_lists.push_back(off | (cap << 16));
            off += 2u * (1u + cap);
        }
        body_end = (size_t)C0.ere_off_fw + off;
        for (uint32_t n = 0; n < N; ++n) {
            const mcbs_node_static* nsn = reinterpret_cast<const mcbs_node_static*>(topo->host.data() + h->off_node) + n;
            if (nsn->svc_cnt > 32) { delete b; return fail(MCBS_ELIMIT, "node %u has more than 32 services", n); }
        }
    }
    S.body_stride = (uint32_t)align_up(body_end, S.packed ? 16 : 64);

    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };
    const size_t o_h0 = take(16ull * E), o_h1 = take(16ull * E), o_ep = take(4ull * E), o_pend = take(8ull * E);
    uint32_t wt = S.NW > S.SW ? S.NW : S.SW;
    S.wide = S.TW > 4u ? 1u : 0u;             // the cached-triple set does not fit 4 words: own column array (DevState::cach)
    if (!S.wide && S.TW > wt) wt = S.TW;
    S.WT = wt <= 1 ? 1 : (wt == 2 ? 2 : 4);
    const size_t o_masks = take(S.packed ? 32ull * E : 8ull * M_COUNT * S.WT * E);   // packed: the sets column, then the lists-word column
    const size_t o_cach = S.wide ? take(8ull * S.TW * E) : 0;
    const bool has_def = cfg->defender_kind != MCBS_DEFENDER_NONE;   // in-env or external: both re-image nodes
    const size_t o_ring = has_def ? take(8ull * 16 * S.WT * E) : 0;
    const size_t o_init = take(S.body_stride);
    const size_t o_digest = take(sizeof(ObsDigest) * (size_t)E);
    const size_t o_rdigest = take(sizeof(ObsDigest));
    const size_t o_body = take((size_t)S.body_stride * E + 64);   // + 64: packed batches fetch a fixed 64 bytes of rows per env
    b->arena_bytes = off;

    DeviceGuard guard(cfg->device);
    hipError_t e = guard.err;
    if (e == hipSuccess) e = hipMalloc(&b->arena, b->arena_bytes);
    if (e != hipSuccess) { delete b; return fail(MCBS_EHIP, "state allocation of %zu bytes failed: %s", off, hipGetErrorString(e)); }
    uint8_t* a = b->arena;
    S.h0 = reinterpret_cast<uint4*>(a + o_h0); S.h1 = reinterpret_cast<double2*>(a + o_h1);
    S.episode = reinterpret_cast<uint32_t*>(a + o_ep); S.pending = reinterpret_cast<double*>(a + o_pend);
    S.masks = reinterpret_cast<uint64_t*>(a + o_masks);
    S.cach = S.wide ? reinterpret_cast<uint64_t*>(a + o_cach) : nullptr;
    S.ring = has_def ? reinterpret_cast<uint64_t*>(a + o_ring) : nullptr;
    S.body = a + o_body; S.init_body = a + o_init;
    b->digest = reinterpret_cast<ObsDigest*>(a + o_digest);
    b->reset_digest = reinterpret_cast<ObsDigest*>(a + o_rdigest);
    b->T.base = topo->dev;
    b->T.hot = topo->hot_dev;

    // reset image of one env body: rows of the initially owned nodes know all their properties and carry
    // max(initial privilege, LocalUser) (actions.py:149-152,263-270); every row carries its literal tags
    std::vector<uint8_t> init(S.body_stride, 0);
    const mcbs_node_static* ns = reinterpret_cast<const mcbs_node_static*>(topo->host.data() + h->off_node);
    for (uint32_t n = 0; n < N; ++n) {
        Row r{};
        const bool owned0 = (ns[n].flags & MCBS_NODE_INSTALLED0) != 0;
        r.props_tags = (owned0 ? ns[n].props : 0ull) | ((uint64_t)(ns[n].tags0 & 0xFu) << 60);
        S.row_put(init.data(), n, r);
    }
    if (!S.packed) memcpy(init.data() + S.off_disc, topo->host.data() + h->off_init_order, h->n_init_owned);
    if (external) memcpy(init.data() + S.off_fw, topo->host.data() + h->off_fw_list0, 2u * h->n_fw_lists);
    if (random_events) {
        const uint8_t* tb = topo->host.data();
        const mcbs_ere_tables* et = reinterpret_cast<const mcbs_ere_tables*>(tb + h->off_ere);
        const uint8_t* own_keys = reinterpret_cast<const uint8_t*>(et) + et->off_own_keys;
        const uint8_t* own_cnt = reinterpret_cast<const uint8_t*>(et) + et->off_own_cnt;
        const mcbs_service* sv0 = reinterpret_cast<const mcbs_service*>(tb + h->off_service);
        memcpy(init.data() + b->C.ere_off_keys, own_keys, (size_t)et->key_cap * N);
        memcpy(init.data() + b->C.ere_off_kcnt, own_cnt, N);
        for (uint32_t n = 0; n < N; ++n) {
            uint64_t present = 0;
            for (uint32_t k = 0; k < own_cnt[n]; ++k) present |= 1ull << own_keys[(size_t)n * et->key_cap + k];
            memcpy(init.data() + b->C.ere_off_present + 8u * n, &present, 8);
            uint32_t run = 0;
            for (uint32_t i = 0; i < ns[n].svc_cnt; ++i) if (sv0[ns[n].svc_off + i].running) run |= 1u << i;
            memcpy(init.data() + b->C.ere_off_svc + 4u * n, &run, 4);
        }
        const mcbs_fw_rule* fwr = reinterpret_cast<const mcbs_fw_rule*>(tb + h->off_fw_rule);
        const uint16_t* fr = reinterpret_cast<const uint16_t*>(tb + h->off_fw_range);
        for (uint32_t l = 0; l < h->n_fw_lists; ++l) {
            uint16_t* L = reinterpret_cast<uint16_t*>(init.data() + b->C.ere_off_fw + (ere_lists[l] & 0xFFFFu));
            L[0] = fr[l * 2 + 1];
            for (uint32_t i = 0; i < fr[l * 2 + 1]; ++i) L[1 + i] = (uint16_t)(fwr[fr[l * 2] + i].name | ((fwr[fr[l * 2] + i].allow ? 1u : 0u) << 8));
        }
        hipError_t e2 = hipMalloc(&b->ere_lists_dev, sizeof(uint32_t) * (ere_lists.size() + 1));
        if (e2 == hipSuccess) e2 = hipMemcpy(b->ere_lists_dev, ere_lists.data(), sizeof(uint32_t) * ere_lists.size(), hipMemcpyHostToDevice);
        if (e2 != hipSuccess) { (void)hipFree(b->arena); delete b; return fail(MCBS_EHIP, "random-events tables upload failed: %s", hipGetErrorString(e2)); }
        b->C.ere_lists = b->ere_lists_dev;
    }
    e = hipMemcpy(a + o_init, init.data(), init.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(b->arena); delete b; return fail(MCBS_EHIP, "init image upload failed: %s", hipGetErrorString(e)); }

    StepCfg& C = b->C;
    C.goal_reward = cfg->goal_reward; C.goal_low_availability = cfg->goal_low_availability;
    C.goal_own_atleast_percent = cfg->goal_own_atleast_percent; C.maintain_sla = cfg->maintain_sla;
    C.goal_own_pct_min = N + 1u;
    for (uint32_t k = 0; k <= N; ++k)
        if (!((double)k / (double)N < cfg->goal_own_atleast_percent)) { C.goal_own_pct_min = k; break; }     // (monotone in k: N > 0)
    C.winning_reward = cfg->winning_reward; C.losing_reward = cfg->losing_reward; C.scan_probability = cfg->scan_probability;
    C.total_sla_weight = h->total_sla_weight; C.full_availability = h->full_availability; C.full_sum = h->full_sum;
    C.seed = cfg->seed; C.env_id_base = cfg->env_id_base;
    C.has_attacker_goal = cfg->has_attacker_goal; C.goal_own_atleast = cfg->goal_own_atleast;
    C.defender_goal_eviction = cfg->defender_goal_eviction; C.defender_kind = cfg->defender_kind;
    C.scan_capacity = cfg->scan_capacity; C.scan_frequency = cfg->scan_frequency ? cfg->scan_frequency : 1;
    C.auto_reset = cfg->auto_reset; C.max_episode_steps = cfg->max_episode_steps; C.rng_kind = cfg->rng_kind;
    C.avail_any_order = h->avail_any_order;
    C.L = h->n_local; C.R = h->n_remote; C.P = h->n_ports; C.V = h->max_slots; C.n_props = h->n_props;
    C.K = cfg->maximum_discoverable_credentials_per_action;
    C.off_node = h->off_node; C.off_slot_of = h->off_slot_of; C.off_slot = h->off_slot; C.off_payload = h->off_payload;
    C.off_service = h->off_service; C.off_allowed = h->off_allowed; C.off_triple = h->off_triple;
    C.hot_node = topo->hot.node; C.hot_desc = topo->hot.desc; C.hot_payload = topo->hot.payload; C.hot_auth = topo->hot.auth;
    memcpy(C.rule_port, h->rule_port, 8); C.n_services = h->n_services; C.n_fw_lists = h->n_fw_lists; C.hot_fwlist = topo->hot.fwlist;
    C.max_leak = topo->hot.max_leak;
    C.auth_words = topo->hot.auth_words; C.hot_triple = topo->hot.triple; C.hot_avail = topo->hot.avail; C.hot_bytes = topo->hot.bytes;
    C.avail_uniform = h->avail_any_order ? 1u : 0u;
    C.avail_term0 = ns[0].avail_term;
    for (uint32_t n = 0; n < N; ++n) {
        if (ns[n].flags & MCBS_NODE_REIMAGABLE) C.reimagable[n >> 6] |= 1ull << (n & 63u);
        if (ns[n].avail_term != ns[0].avail_term) C.avail_uniform = 0u;
    }

    C.n_init = h->n_init_owned;
    if (S.packed && S.body_stride <= sizeof(C.init_image)) {
        C.init_image_ok = 1u;
        memcpy(C.init_image, init.data(), S.body_stride);
        uint16_t f[M_COUNT] = {0, 0, 0, 0, 0, 0, 0, 0};
        const uint8_t* order0 = topo->host.data() + h->off_init_order;
        for (uint32_t i = 0; i < h->n_init_owned; ++i) {
            const uint32_t n = order0[i];
            f[M_DISC] |= 1u << n; f[M_INST] |= 1u << n; f[M_EVER] |= 1u << n;
            if (ns[n].priv0 & 1u) f[M_PLO] |= 1u << n;
            if (ns[n].priv0 & 2u) f[M_PHI] |= 1u << n;
        }
        f[M_RUN] = (uint16_t)((1u << N) - 1u);
        for (int q = 0; q < 4; ++q) C.init_packed[q] = (uint32_t)f[2 * q] | ((uint32_t)f[2 * q + 1] << 16);
        uint64_t dl = 0;                                           // the lists word of a fresh env (reset_header builds the same one)
        for (uint32_t i = 0; i < h->n_init_owned && i < 16u; ++i) dl |= (uint64_t)(order0[i] & 0xFu) << (4u * i);
        C.init_lists[0] = (uint32_t)dl; C.init_lists[1] = (uint32_t)(dl >> 32); C.init_lists[2] = C.init_lists[3] = 0u;
    }

    e = hipMalloc(&b->C_dev, sizeof(StepCfg));
    if (e == hipSuccess) e = hipMemcpy(b->C_dev, &b->C, sizeof(StepCfg), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(b->arena); delete b; return fail(MCBS_EHIP, "config upload failed: %s", hipGetErrorString(e)); }
    if (external) {
        // the packed defender observation (mcbs_defender_obs_packing.hip): services never change state, so their bits of a row are built here, once
        DefPackGeom& P = b->def_pack;
        P.N = N; P.S = h->n_services; P.F = 13u * N + P.S; P.W = (P.F + 31u) / 32u;
        P.dW = fast_div_host(P.W ? P.W : 1u);
        std::vector<uint32_t> image(P.W ? P.W : 1u, 0u);
        const mcbs_service* sv = reinterpret_cast<const mcbs_service*>(topo->host.data() + h->off_service);
        for (uint32_t k = 0; k < P.S; ++k)
            if (sv[k].running) image[(13u * N + k) >> 5] |= 1u << ((13u * N + k) & 31u);
        uint32_t* dev = nullptr;
        e = hipMalloc(&dev, image.size() * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMemcpy(dev, image.data(), image.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            if (dev) (void)hipFree(dev);
            (void)hipFree(b->C_dev); (void)hipFree(b->arena); delete b;
            return fail(MCBS_EHIP, "services image upload failed: %s", hipGetErrorString(e));
        }
        P.svc = dev;
    }
    launch_step_zero(b, nullptr, 0, nullptr);
    e = hipDeviceSynchronize();
    if (e != hipSuccess) { (void)hipFree(b->arena); delete b; return fail(MCBS_EHIP, "initial reset failed: %s", hipGetErrorString(e)); }
    b->variant = batch_variant(b);
    b->lean_step = S.packed && cfg->defender_kind == MCBS_DEFENDER_NONE && C.init_image_ok && !S.ring;
    // (the narrow kernel fetches the fourth row vector where body_stride > 48: a lean body is its 4-byte rows alone, so that is N > 12)
    b->narrow_step = b->lean_step && !(topo->hot.traits & ~kNarrowStepCan) && ((S.N > 12u) == (S.body_stride > 48u));
    *out = b;
    return MCBS_OK;
}

extern "C" void mcbs_batch_destroy(mcbs_batch* b) {
    if (!b) return;
    DeviceGuard guard(b->cfg.device);
    for (hipEvent_t ev : b->ev) (void)hipEventDestroy(ev);
    if (b->arena) (void)hipFree(b->arena);
    if (b->C_dev) (void)hipFree(b->C_dev);
    if (b->ere_lists_dev) (void)hipFree(b->ere_lists_dev);
    if (b->def_pack.svc) (void)hipFree(const_cast<uint32_t*>(b->def_pack.svc));
    delete b;
}

static int launch_ok(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MCBS_EHIP, "%s launch failed: %s", what, hipGetErrorString(e));
    return MCBS_OK;
}

extern "C" int mcbs_reset(mcbs_batch* b, const uint8_t* env_mask, void* stream) {
    if (!b) return fail(MCBS_EINVAL, "null batch");
    MCBS_ON_DEVICE(b);
    launch_step_zero(b, env_mask, 1, (hipStream_t)stream);
    if (!env_mask) b->all_fresh = true;
    b->digest_state = !env_mask ? 0 : (b->digest_state == 1 ? 2 : b->digest_state);
    return launch_ok("reset");
}

extern "C" int mcbs_rewind(mcbs_batch* b, void* stream) {
    if (!b) return fail(MCBS_EINVAL, "null batch");
    MCBS_ON_DEVICE(b);
    launch_step_zero(b, nullptr, 0, (hipStream_t)stream);
    b->all_fresh = true;
    b->digest_state = 0;
    return launch_ok("rewind");
}

extern "C" int mcbs_set_mask_discrete_stride(mcbs_batch* b, size_t stride_bytes) {
    if (!b) return fail(MCBS_EINVAL, "null batch");
    if (stride_bytes && stride_bytes < mcbs_discrete_action_count(b)) return fail(MCBS_EINVAL, "row stride shorter than the Discrete action count");
    b->disc_stride = stride_bytes;
    return MCBS_OK;
}

extern "C" int mcbs_set_draw_tape(mcbs_batch* b, const double* tape, uint32_t draws_per_step) {
    if (!b) return fail(MCBS_EINVAL, "null batch");
    b->tape = tape;
    b->tape_dps = tape ? draws_per_step : 0;
    return MCBS_OK;
}

static StepIO make_io(mcbs_batch* b, const int32_t* actions, float* reward, uint8_t* terminated, const mcbs_info_buffers* info) {
    StepIO io{};
    io.actions = actions; io.reward = reward; io.terminated = terminated;
    if (info) {
        io.availability = info->network_availability; io.step_count = info->step_count; io.truncated = info->truncated;
        io.oob = info->out_of_bound; io.raw_reward = info->raw_reward;
    }
    io.tape = b->tape; io.tape_dps = b->tape_dps;
#ifdef MCBS_DIAG
    io.stamps = b->stamps;
#endif
    // Kernel-argument budget: DevState + Topo + config pointer + StepIO are followed by the hidden launch arguments; the block
    // size the kernel reads first sits 12 bytes in.  When that crossed byte 256 the step took 5.73 instead of 5.47 us — a step
    // function (64 or 128 bytes more cost the same), as if only the first 256 bytes of the arguments are prefetched for the waves.
#ifndef MCBS_DIAG
    static_assert(sizeof(DevState) + sizeof(Topo) + sizeof(void*) + sizeof(StepIO) + 16 <= 256, "step kernel arguments spill into a fifth cache line");
#endif
    return io;
}

static int timing_begin(mcbs_batch* b, hipStream_t st, size_t* slot) {
    *slot = (size_t)-1;
    if (!b->timing) return MCBS_OK;
    if (b->ev_used + 2 > b->ev.size()) {
        for (int i = 0; i < 2; ++i) { hipEvent_t ev; HIP_TRY(hipEventCreate(&ev)); b->ev.push_back(ev); }
    }
    *slot = b->ev_used;
    b->ev_used += 2;
    HIP_TRY(hipEventRecord(b->ev[*slot], st));
    return MCBS_OK;
}

static int timing_end(mcbs_batch* b, hipStream_t st, size_t slot) {
    if (slot == (size_t)-1) return MCBS_OK;
    HIP_TRY(hipEventRecord(b->ev[slot + 1], st));
    return MCBS_OK;
}

// Value -> template argument: calls f(std::integral_constant<int, V>{}) for the V among Vs that equals v, and for the LAST V when none
// does (the else arm of the if / else ladders this replaces).  A call site lists exactly the values it may instantiate kernels for.
template <int V, int... Vs, class F>
static void pick(int v, F&& f) {
    if constexpr (sizeof...(Vs) == 0) f(std::integral_constant<int, V>{});
    else if (v == V) f(std::integral_constant<int, V>{});
    else pick<Vs...>(v, f);
}

// The step family's variant: f(WT, DEF) with WT = words per set kept in registers (1, 2 or 4; 0 = packed batch: one word of registers
// each) and DEF = the configured defender (its code and loads are compiled out otherwise)
template <class F>
static void step_variant(const mcbs_batch* b, F&& f) {
    pick<0, 1, 2, 4>(b->S.packed ? 0 : (int)b->S.WT, [&](auto wt) {
        pick<MCBS_DEFENDER_SCAN_AND_REIMAGE, MCBS_DEFENDER_RANDOM_EVENTS, MCBS_DEFENDER_EXTERNAL, MCBS_DEFENDER_NONE>(
            (int)b->cfg.defender_kind, [&](auto def) { f(wt, def); });
    });
}

// Launch shape of every kernel built on step_body (mcbs_step.hip): one lane per env in one-wavefront workgroups — fixed, the kernels rely
// on it; beyond one wavefront per SIMD the shape no longer matters: 22.7 (64) vs 22.2 us (256 threads) at 131 072 Random-256 envs —
// and, as dynamic LDS, the lanes' columns of a wide cached-triple set.  The topology's hot image is read through L1 / L2: a copy in LDS
// per workgroup measured slower at every BASELINE shape in rounds 2 and 3 (profiles/step_dispatch_refactor.md) and is gone.
static dim3 step_grid(const mcbs_batch* b) { return dim3((b->S.E + 63u) / 64u); }
static uint32_t step_lds(const mcbs_batch* b) { return b->S.wide ? 64u * b->S.TW * 8u : 0u; }

template <int PHASE, bool MANY = false>
static int launch_step(mcbs_batch* b, const StepIO& io, hipStream_t st, const char* what, const RollArgs& roll = RollArgs{}) {
    b->all_fresh = false;
    if (PHASE == 0 && !MANY && b->variant.coop) {           // G = WT lanes per env, G envs fewer per wavefront
        pick<2, 4>((int)b->S.WT, [&](auto g) {
            pick<MCBS_DEFENDER_SCAN_AND_REIMAGE, MCBS_DEFENDER_NONE>((int)b->cfg.defender_kind, [&](auto def) {
                constexpr uint32_t epw = 64u / decltype(g)::value;
                hipLaunchKernelGGL((step_coop_kernel<decltype(g)::value, decltype(def)::value>), dim3((b->S.E + epw - 1u) / epw), dim3(64), 0, st,
                                   b->S, b->T, b->C_dev, io);
            });
        });
        return launch_ok(what);
    }
    if (PHASE == 0 && !MANY && b->lean_step && !(io.availability || io.step_count || io.truncated || io.oob || io.raw_reward)) {
        // no info buffers on a packed, attacker-only batch: the same kernel with the argument block that holds only what it reads
        const DevState& S = b->S;
        LeanStepArgs a{};
        a.h0 = S.h0; a.masks = S.masks; a.body = S.body; a.h1 = S.h1; a.actions = io.actions; a.reward = io.reward; a.terminated = io.terminated;
        a.E = S.E; a.body_stride = S.body_stride; a.hot = b->T.hot; a.N = S.N; a.tiny_p = S.tiny_p; a.tiny_v = S.tiny_v;
        a.episode = S.episode; a.pending = S.pending;
        static_assert(sizeof(LeanStepArgs) + sizeof(void*) + 16 <= 256, "step kernel arguments spill into a fifth cache line (make_io)");
#ifdef MCBS_DIAG
        a.stamps = io.stamps;
#endif
        // ... instantiated for what the batch's topology can do, where that is no more than the narrow kernel handles: a kernel built
        // in a translation unit of its own (mcbs_step_narrow_tu.hip), whose argument list is this block's members but N
        if (b->narrow_step) launch_step_narrow(step_grid(b), st, b->C_dev, b->C, a);
        else hipLaunchKernelGGL((step_kernel<0, 0, false, MCBS_DEFENDER_NONE>), step_grid(b), dim3(64), 0, st, b->C_dev, a);
        return launch_ok(what);
    }
    step_variant(b, [&](auto wt, auto def) {
        constexpr int WT = decltype(wt)::value, DEF = decltype(def)::value;
        if constexpr (MANY) hipLaunchKernelGGL((step_many_kernel<WT, false, DEF>), step_grid(b), dim3(64), step_lds(b), st, b->S, b->T, b->C_dev, io, roll);
        else hipLaunchKernelGGL((step_kernel<PHASE, WT, false, DEF>), step_grid(b), dim3(64), step_lds(b), st, b->S, b->T, b->C_dev, io);
    });
    return launch_ok(what);
}

// A step launch between the two event records of mcbs_timing_enable
template <bool MANY>
static int launch_step_timed(mcbs_batch* b, const StepIO& io, hipStream_t st, const char* what) {
    size_t slot;
    int rc = timing_begin(b, st, &slot);
    if (rc) return rc;
    if ((rc = launch_step<0, MANY>(b, io, st, what))) return rc;
    return timing_end(b, st, slot);
}

// The in-env defender's draws of a MCBS_RNG_TAPE batch come from the caller's tape, one step's worth: a single step needs the tape to
// have been set; the entry point `many` (several steps per launch) cannot run from a tape at all
static int draws_ok(const mcbs_batch* b, const char* many = nullptr) {
    if (b->cfg.rng_kind != MCBS_RNG_TAPE || b->cfg.defender_kind == MCBS_DEFENDER_NONE) return MCBS_OK;
    if (many) return fail(MCBS_ESTATE, "%s needs the Philox generator: a draw tape holds one step's draws", many);
    return b->tape ? MCBS_OK : fail(MCBS_ESTATE, "rng_kind is TAPE but no draw tape was set (mcbs_set_draw_tape)");
}

extern "C" int mcbs_step(mcbs_batch* b, const int32_t* actions, float* reward, uint8_t* terminated,
                         const mcbs_info_buffers* info, void* stream) {
    if (!b || !actions || !reward || !terminated) return fail(MCBS_EINVAL, "null argument");
    MCBS_ON_DEVICE(b);
    if (const int rc = draws_ok(b)) return rc;
    return launch_step_timed<false>(b, make_io(b, actions, reward, terminated, info), (hipStream_t)stream, "step");
}

// n_steps consecutive steps in one launch: scripted / recorded / pre-sampled action sequences (replaying a trace, random-agent
// baselines, evaluating fixed plans), where nothing has to be observed between steps.  Results are those of n_steps calls of
// mcbs_step; what is saved is the per-launch cost between dependent launches (1.5 us of a 5.5 us step at 65 536 envs).
extern "C" int mcbs_step_many(mcbs_batch* b, const int32_t* actions, float* reward, uint8_t* terminated, uint32_t n_steps, void* stream) {
    if (!b || !actions || !reward || !terminated) return fail(MCBS_EINVAL, "null argument");
    MCBS_ON_DEVICE(b);
    if (n_steps == 0) return MCBS_OK;
    if (const int rc = draws_ok(b, "mcbs_step_many")) return rc;
    StepIO io = make_io(b, actions, reward, terminated, nullptr);
    io.n_steps = n_steps;
    return launch_step_timed<true>(b, io, (hipStream_t)stream, "step (many)");
}

// Random agents entirely on the device: every step's action is drawn from the env's own state inside the step kernel
// (sample_action, the distribution of CyberBattleEnv.sample_valid_action or uniform over the action space), K steps per launch.
// This is marlon.simulate's loop for random agents (marlon/simulate.py:14-35) without a launch per sample and per step.
extern "C" int mcbs_rollout_random(mcbs_batch* b, int32_t valid, uint64_t seed, uint64_t first_step, uint32_t n_steps,
                                   int32_t* actions_out, float* reward, uint8_t* terminated, void* stream) {
    if (!b || !reward || !terminated) return fail(MCBS_EINVAL, "null argument");
    MCBS_ON_DEVICE(b);
    if (n_steps == 0) return MCBS_OK;
    if (const int rc = draws_ok(b, "mcbs_rollout_random")) return rc;
    hipStream_t st = (hipStream_t)stream;
    RollArgs roll;
    roll.mode = valid ? 2u : 1u; roll.nmax = b->cfg.maximum_node_count; roll.cmax = b->cfg.maximum_total_credentials;
    roll.seed = seed; roll.step0 = first_step;
    StepIO io = make_io(b, actions_out, reward, terminated, nullptr);
    io.n_steps = n_steps;
    return launch_step<0, true>(b, io, st, "rollout", roll);   // the random agent's parameters are kernel arguments: no host copy, no shared state
}

static int launch_masks(mcbs_batch* b, const mcbs_obs_buffers* o, hipStream_t st, const uint8_t* env_mask, bool masks_only);

// The first whole-batch observation after a whole-batch reset also keeps env 0's digest as "the digest of a freshly reset env"
// (mcbs_attacker_wrapper_finish hands it to the envs it resets): one 64-byte device copy, once per batch.
static int capture_reset_digest(mcbs_batch* b, hipStream_t st, bool whole_batch) {
    if (!whole_batch || !b->all_fresh || b->reset_digest_ok) return MCBS_OK;
    HIP_TRY(hipMemcpyAsync(b->reset_digest, b->digest, sizeof(ObsDigest), hipMemcpyDeviceToDevice, st));
    b->reset_digest_ok = true;
    return MCBS_OK;
}

static int launch_obs_inner(mcbs_batch* b, const mcbs_obs_buffers* o, hipStream_t st, bool masks_only, const uint8_t* env_mask);
static int launch_obs(mcbs_batch* b, const mcbs_obs_buffers* o, hipStream_t st, bool masks_only = false, const uint8_t* env_mask = nullptr) {
    const int rc = launch_obs_inner(b, o, st, masks_only, env_mask);
    if (rc) return rc;
    if (!env_mask) b->digest_lists = false;                   // every digest rewritten, none with a list of its own
    if (!env_mask) b->digest_state = 1;                       // every observation kernel (masks-only ones too) leaves the env's digest
    else if (b->digest_state == 2) b->digest_state = 1;       // the envs reset by mask have been re-observed (the caller's protocol)
    return capture_reset_digest(b, st, !masks_only && !env_mask);
}

static int launch_obs_inner(mcbs_batch* b, const mcbs_obs_buffers* o, hipStream_t st, bool masks_only, const uint8_t* env_mask) {
    ObsIO O{};
    O.masks_only = masks_only ? 1u : 0u;
    O.env_mask = env_mask;
    O.scalars = o->scalars; O.leaked = o->leaked_credentials; O.cache_matrix = o->credential_cache_matrix;
    O.props = o->discovered_nodes_properties; O.priv = o->nodes_privilegelevel; O.mask_local = o->mask_local;
    O.mask_remote = o->mask_remote; O.mask_connect = o->mask_connect; O.mask_discrete = o->mask_discrete;
    O.Nmax = b->cfg.maximum_node_count; O.Cmax = b->cfg.maximum_total_credentials; O.K = b->cfg.maximum_discoverable_credentials_per_action;
    // small action spaces: the per-env wavefront also writes mask_remote / mask_connect (mcbs_obs.hip)
    const size_t rows = (size_t)O.Nmax * O.Nmax, RL = (size_t)b->C.P * O.Cmax;
    const bool small = rows <= 256 && !b->no_fused_masks;
    O.fuse_remote = small && o->mask_remote && (rows * b->C.R) % 4 == 0 && reinterpret_cast<uintptr_t>(o->mask_remote) % 4 == 0;
    const size_t ML = (size_t)O.Nmax * b->C.L, MR = rows * b->C.R, M = rows * RL;
    const bool dwords_ok = small && RL >= 4 && RL + 4 <= 1040 && M % 4 == 0;     // the row pattern fits its kilobyte of LDS
    O.fuse_connect = 0;
    if (small && o->mask_connect) {
        size_t g16 = 16;
        while (RL % g16) g16 >>= 1;                                                                                          // gcd(RL, 16)
        if (RL % 16 == 0 && RL / 16 <= 64 && reinterpret_cast<uintptr_t>(o->mask_connect) % 16 == 0) O.fuse_connect = 1;   // 16-byte chunks
        else if (RL >= 16 && RL / g16 <= 64 && M % 16 == 0 && reinterpret_cast<uintptr_t>(o->mask_connect) % 16 == 0 && !b->slow_masks) {
            O.fuse_connect = 3; O.conn_pc = (uint32_t)(RL / g16);                                                            // 16-byte chunks, any RL >= 16
        } else if (dwords_ok && reinterpret_cast<uintptr_t>(o->mask_connect) % 4 == 0) O.fuse_connect = 2;                  // dwords, any RL
    }
    // per-source blocks (mcbs_obs.hip stream_blocks): where round 2 switched row bytes on and off per chunk (connect rows that are not a
    // multiple of 16 bytes; the remote mask as dwords), a chunk is now one LDS read of a block variant.  Needs dword-sized blocks of at
    // least one chunk and whole-chunk masks; MCBS_NO_BLOCK_MASKS=1: round 2's writers
    uint32_t blk_bytes = 0;
    const size_t BLc = (size_t)O.Nmax * RL, BLr = (size_t)O.Nmax * b->C.R;
    // largest block whose four variants still fit a workgroup's LDS next to the staging areas (four wavefronts, 60 KB in all, 4 KB of it
    // obs_quad_kernel's static arrays): 3 161 bytes for a 16-node topology, less when the credential lists are long
    size_t blk_cap = 0;
    {
        const size_t fixed = obs_stage_bytes(b->S.N, b->topo->H()->n_triples, 0), budget = (61440u - 4096u) / 4u;
        if (budget > fixed + 16u * 12u) blk_cap = ((budget - fixed) / 16u) * 4u - 31u;
        if (blk_cap > 4064u) blk_cap = 4064u;
    }
    if (!b->no_block_masks) {
        if (O.fuse_connect == 3 && BLc % 4 == 0 && BLc >= 16 && BLc <= blk_cap) { O.fuse_connect = 4; blk_bytes = (uint32_t)BLc; }
        if (O.fuse_remote && BLr % 4 == 0 && BLr >= 16 && BLr <= blk_cap && MR % 16 == 0 && reinterpret_cast<uintptr_t>(o->mask_remote) % 16 == 0) {
            O.fuse_remote = 2;
            if (BLr > blk_bytes) blk_bytes = (uint32_t)BLr;
        }
    }
    O.fuse_discrete = dwords_ok && o->mask_discrete && ML % 4 == 0 && MR % 4 == 0 && b->C.L > 0 && b->C.R > 0 &&
                      reinterpret_cast<uintptr_t>(o->mask_discrete) % 4 == 0;
    {   // row stride of mask_discrete: dense unless the caller padded its rows (mcbs_set_mask_discrete_stride)
        const size_t D = M + ML + MR, stride = b->disc_stride ? b->disc_stride : D;
        if (stride > 0xFFFFFFFFull) return fail(MCBS_ELIMIT, "mask_discrete row stride too large");
        O.disc_stride = (uint32_t)stride;
        if (O.fuse_discrete && stride % 4 != 0) O.fuse_discrete = 0;
        O.nt_discrete = (O.fuse_discrete && stride % 128 == 0 && reinterpret_cast<uintptr_t>(o->mask_discrete) % 128 == 0 && M % 128 == 0) ? 1u : 0u;
    }
    O.disc_blocks = (!b->no_block_masks && O.fuse_discrete && RL % 16 != 0 && BLc % 4 == 0 && BLc >= 16 && BLc <= blk_cap) ? 1u : 0u;
    if (O.disc_blocks && BLc > blk_bytes) blk_bytes = (uint32_t)BLc;
    O.disc_remote_blocks = (!b->no_block_masks && O.fuse_discrete && BLr % 4 == 0 && BLr >= 16 && BLr <= blk_cap) ? 1u : 0u;
    if (O.disc_remote_blocks && BLr > blk_bytes) blk_bytes = (uint32_t)BLr;
    O.blk_region = blk_bytes ? ((blk_bytes + 16u + 15u) / 16u) * 4u : 0u;
    O.dBLc = fast_div_host(BLc ? (uint32_t)BLc : 1u); O.dBLr = fast_div_host(BLr ? (uint32_t)BLr : 1u);
    O.nt_connect = (O.fuse_connect == 1 && M % 128 == 0 && reinterpret_cast<uintptr_t>(o->mask_connect) % 128 == 0) ? 1u : 0u;
    auto fdh = [](size_t d) { return fast_div_host(d ? (uint32_t)d : 1u); };
    O.dNP = fdh(b->C.n_props); O.dL = fdh(b->C.L); O.dR = fdh(b->C.R); O.dNm = fdh(O.Nmax); O.dRL = fdh(RL); O.dC = fdh(O.Cmax);
    O.dPC = fdh(O.conn_pc); O.dCPR = fdh(RL >> 4);
    const uint32_t obs_shm = 4u * obs_stage_bytes(b->S.N, b->topo->H()->n_triples, O.blk_region);
    const bool no_masks = !o->mask_local && !o->mask_remote && !o->mask_connect && !o->mask_discrete;
    const bool groups_ok = !env_mask && !masks_only && b->S.NW == 1u && b->S.N <= 16u && O.Nmax <= 16u && O.Cmax <= 16u &&
                           b->topo->H()->n_triples <= 15u && b->cfg.defender_kind != MCBS_DEFENDER_RANDOM_EVENTS && !b->no_fused_masks;
    if (groups_ok && no_masks) {
        // ~1 KB per env, no mask field: sixteen lanes per env instead of a wavefront (mcbs_obs.hip obs_tiny_kernel)
        hipLaunchKernelGGL(obs_tiny_kernel, dim3((b->S.E + 15u) / 16u), dim3(256), 0, st, b->S, b->T, b->C_dev, O, b->digest);
        return launch_ok("obs_tiny");
    }
    // ... with mask fields: the small fields by 16-lane groups, the masks of the wavefront's four envs one after the other (obs_quad_kernel).
    // Measured (tools/obs_field_matrix.py, profiles/round3_notes.md section 7): ToyCtf's whole observation 43 -> 40 us at 16 384 envs and
    // 190 -> 145 us at 65 536 (its 10 080-byte mask rows share cache lines with their neighbours, and four envs' small fields go out in one
    // store instead of four partial lines); Chain-10, whose mask rows are whole 128-byte lines written with non-temporal stores, streams
    // ~10 % FASTER with a wavefront per env (152-168 against 171-185 us at 65 536 envs) and keeps it.  MCBS_QUAD_OBS=1 / MCBS_NO_QUAD_OBS=1
    // force one or the other.
    // The flat Discrete mask of a batch too small to give every SIMD several four-env wavefronts also stays (ToyCtf, 16 384 envs: 50 us
    // against 52-54; 65 536 envs: 207 -> 171 us).
    const bool line_rows = (o->mask_connect && O.nt_connect) || (o->mask_discrete && O.nt_discrete);
    const bool few_waves = o->mask_discrete && b->S.E < 32768u;
    if (groups_ok && !b->no_quad_obs && ((!line_rows && !few_waves) || b->force_quad_obs)) {
        const uint32_t quad_shm = 4u * (272u + 1040u + 16u * O.blk_region);
        hipLaunchKernelGGL(obs_quad_kernel, dim3((b->S.E + 15u) / 16u), dim3(256), quad_shm, st, b->S, b->T, b->C_dev, O, b->digest);
    } else if (env_mask) {     // sparse by nature (the envs a VecEnv just reset): 64 envs' mask bytes per wavefront
        const uint32_t waves = (b->S.E + 63u) / 64u;
        hipLaunchKernelGGL(obs_scan_kernel, dim3((waves + 3u) / 4u), dim3(256), obs_shm, st, b->S, b->T, b->C_dev, O, b->digest);
    } else {
        hipLaunchKernelGGL(obs_small_kernel, dim3((b->S.E + 3) / 4), dim3(256), obs_shm, st, b->S, b->T, b->C_dev, O, b->digest);
    }
    int rc = launch_ok("obs_small");
    if (rc) return rc;
    mcbs_obs_buffers rest = *o;                // what the fused wavefront has not written
    if (O.fuse_remote) rest.mask_remote = nullptr;
    if (O.fuse_connect) rest.mask_connect = nullptr;
    if (O.fuse_discrete) rest.mask_discrete = nullptr;
    return launch_masks(b, &rest, st, env_mask, masks_only);
}

template <int REGION>
static int launch_region(mcbs_batch* b, int8_t* dst, size_t env_stride, size_t region_off, size_t len, hipStream_t st, const uint8_t* env_mask, bool masks_only) {
    const uint32_t Nm = b->cfg.maximum_node_count, Cm = b->cfg.maximum_total_credentials;
    const uintptr_t base = reinterpret_cast<uintptr_t>(dst) + region_off;
    int W = 1;
    if (base % 16 == 0 && env_stride % 16 == 0 && len % 16 == 0) W = 16;
    else if (base % 4 == 0 && env_stride % 4 == 0 && len % 4 == 0) W = 4;
    const size_t chunks = (len + W - 1) / W;
    const dim3 grid(b->S.E, (unsigned)((chunks + 255) / 256));
    if (grid.y > 65535u) return fail(MCBS_ELIMIT, "mask region too large for one launch");
    const uint32_t RL = REGION == 0 ? b->C.P * Cm : (REGION == 1 ? Nm * b->C.R : 0u), Cc = REGION == 0 ? Cm : RL;
    if (W == 16 && REGION == 0 && RL % 16u == 0 && RL >= 16u && !b->slow_masks && !b->no_row_masks) {
        // whole rows of 16-byte chunks: pattern row + per-row on/off bytes in LDS (mcbs_obs.hip: mask_connect_rows_kernel)
        const uint32_t cpr = RL / 16u, rows = Nm * Nm;
        uint32_t rpb = 128u;                                          // rows per workgroup: >= 16 KB of output each
        while (rpb * RL < 16384u && rpb < rows) rpb *= 2u;
        const uint32_t lds = cpr * 16u + ((rpb + 15u) & ~15u);
        if (lds <= 60000u) {
            const uint32_t gx = (rows + rpb - 1u) / rpb;
            uint32_t gy = b->S.E;
            if ((uint64_t)gx * gy > (1u << 20)) gy = (1u << 20) / gx ? (1u << 20) / gx : 1u;
            hipLaunchKernelGGL(mask_connect_rows_kernel, dim3(gx, gy), dim3(256), lds, st, b->S, b->digest, dst, env_stride, region_off,
                               Nm, Cm, RL, rpb, env_mask, masks_only ? 0u : 1u);
            return launch_ok("mask (rows)");
        }
    }
    if (W == 16 && REGION != 2 && RL >= 16u && len < (1ull << 31) && !b->slow_masks) {
        auto fd = [](uint32_t d) { return fast_div_host(d); };
        const uint32_t flat = chunks < 256 && (uint64_t)chunks * b->S.E < (1ull << 31) ? 1u : 0u;
        uint32_t gx = (uint32_t)((chunks + 1023) / 1024 < 8 ? (chunks + 1023) / 1024 : 8);
        uint32_t gy = 4096u / gx;
        if (gy > b->S.E) gy = b->S.E;
        if (flat) { gx = 1; gy = (uint32_t)(((uint64_t)chunks * b->S.E + 255) / 256 < 4096 ? ((uint64_t)chunks * b->S.E + 255) / 256 : 4096); }
        const dim3 fgrid(gx, gy);
        pick<1, 0>((int)flat, [&](auto fl) {
            hipLaunchKernelGGL((mask_fast_kernel<(REGION == 0 ? 0 : 1), decltype(fl)::value != 0>), fgrid, dim3(256), 0, st, b->S, b->digest, dst, env_stride,
                               region_off, (uint32_t)len, RL, Cc, Nm, b->C.R, fd(RL), fd(Cc), fd(Nm), env_mask, masks_only ? 0u : 1u, fd((uint32_t)chunks));
        });
        return launch_ok("mask (fast)");
    }
    pick<16, 4, 1>(W, [&](auto w) {
        hipLaunchKernelGGL((mask_kernel<decltype(w)::value, REGION>), grid, dim3(256), 0, st, b->S, b->T, b->C_dev, b->digest, dst, env_stride, region_off, Nm, Cm,
                           env_mask, masks_only ? 0u : 1u);
    });
    return launch_ok("mask");
}

static int launch_masks(mcbs_batch* b, const mcbs_obs_buffers* o, hipStream_t st, const uint8_t* env_mask, bool masks_only) {
    const size_t Nm = b->cfg.maximum_node_count, Cm = b->cfg.maximum_total_credentials;
    const size_t M = Nm * Nm * b->C.P * Cm, ML = Nm * b->C.L, MR = Nm * Nm * b->C.R;
    int rc = MCBS_OK;
    if (o->mask_connect && (rc = launch_region<0>(b, o->mask_connect, M, 0, M, st, env_mask, masks_only))) return rc;
    if (o->mask_remote && (rc = launch_region<1>(b, o->mask_remote, MR, 0, MR, st, env_mask, masks_only))) return rc;
    if (o->mask_discrete) {   // connect | local | remote (action_masking.py:96-110)
        const size_t D = b->disc_stride ? b->disc_stride : M + ML + MR;       // (env stride; the regions' offsets inside a row are unchanged)
        if ((rc = launch_region<0>(b, o->mask_discrete, D, 0, M, st, env_mask, masks_only))) return rc;
        if ((rc = launch_region<2>(b, o->mask_discrete, D, M, ML, st, env_mask, masks_only))) return rc;
        if ((rc = launch_region<1>(b, o->mask_discrete, D, M + ML, MR, st, env_mask, masks_only))) return rc;
    }
    return rc;
}

extern "C" int mcbs_observe(mcbs_batch* b, const mcbs_obs_buffers* obs, void* stream) {
    if (!b || !obs) return fail(MCBS_EINVAL, "null argument");
    MCBS_ON_DEVICE(b);
    return launch_obs(b, obs, (hipStream_t)stream);
}

extern "C" int mcbs_observe_masked(mcbs_batch* b, const mcbs_obs_buffers* obs, const uint8_t* env_mask, void* stream) {
    if (!b || !obs) return fail(MCBS_EINVAL, "null argument");
    MCBS_ON_DEVICE(b);
    return launch_obs(b, obs, (hipStream_t)stream, false, env_mask);
}

extern "C" int mcbs_action_mask(mcbs_batch* b, const mcbs_obs_buffers* masks, void* stream) {
    if (!b || !masks) return fail(MCBS_EINVAL, "null argument");
    MCBS_ON_DEVICE(b);
    return launch_obs(b, masks, (hipStream_t)stream, true);
}

extern "C" int mcbs_step_observe(mcbs_batch* b, const int32_t* actions, float* reward, uint8_t* terminated,
                                 const mcbs_info_buffers* info, const mcbs_obs_buffers* obs, void* stream) {
    if (!b || !actions || !reward || !terminated || !obs) return fail(MCBS_EINVAL, "null argument");
    MCBS_ON_DEVICE(b);
    int rc = draws_ok(b);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const StepIO io = make_io(b, actions, reward, terminated, info);
    rc = launch_step<1>(b, io, st, "step (attacker phase)");
    if (rc) return rc;
    if ((rc = launch_obs(b, obs, st))) return rc;
    return launch_step<2>(b, io, st, "step (defender phase)");
}

// every pointer member of the buffer struct *w but its last `optional` ones is set
template <class W>
static bool arrays_set(const W* w, size_t optional) {
    const void* const* p = reinterpret_cast<const void* const*>(w);
    for (size_t i = 0; i + optional < sizeof(W) / sizeof(void*); ++i) if (!p[i]) return false;
    return true;
}

extern "C" int mcbs_attacker_wrapper_post(mcbs_batch* b, const mcbs_wrapper_buffers* w, float modifier, int32_t max_timesteps, void* stream) {
    if (!b || !w) return fail(MCBS_EINVAL, "null argument");
    MCBS_ON_DEVICE(b);
    if (!arrays_set(w, 1)) return fail(MCBS_EINVAL, "mcbs_wrapper_buffers: every array but `executed` is required");   // (the last member: not written by this call)
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(w->n_done, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(wrapper_post_kernel, dim3((b->S.E + 255) / 256), dim3(256), 0, st, b->S.E, *w, modifier, max_timesteps);
    return launch_ok("wrapper post");
}

extern "C" int mcbs_attacker_wrapper_clear(mcbs_batch* b, const mcbs_wrapper_buffers* w, void* stream) {
    if (!b || !w || !w->dones || !w->timesteps || !w->valid_action_count || !w->invalid_action_count || !w->episode_returns || !w->has_cyber_reward)
        return fail(MCBS_EINVAL, "null argument");
    MCBS_ON_DEVICE(b);
    hipLaunchKernelGGL(wrapper_clear_kernel, dim3((b->S.E + 255) / 256), dim3(256), 0, (hipStream_t)stream, b->S.E, *w);
    return launch_ok("wrapper clear");
}

extern "C" int mcbs_copy_rows_masked(mcbs_batch* b, const mcbs_row_copies* copies, const uint8_t* env_mask, void* stream) {
    if (!b || !copies || !env_mask) return fail(MCBS_EINVAL, "null argument");
    MCBS_ON_DEVICE(b);
    if (copies->n == 0) return MCBS_OK;
    if (copies->n > 8) return fail(MCBS_EINVAL, "at most eight arrays per call");
    for (uint32_t i = 0; i < copies->n; ++i) if (!copies->src[i] || !copies->dst[i]) return fail(MCBS_EINVAL, "null array");
    const uint32_t waves = (b->S.E + 63u) / 64u;
    hipLaunchKernelGGL(copy_rows_masked_kernel, dim3((waves + 3u) / 4u), dim3(256), 0, (hipStream_t)stream, *copies, env_mask, b->S.E);
    return launch_ok("copy rows");
}

static int finish_args(mcbs_batch* b, const mcbs_wrapper_buffers* w, float modifier, int32_t max_timesteps, int32_t auto_reset,
                       const mcbs_row_copies* keep, const mcbs_row_copies* fresh, WrapperFinishArgs* A) {
    if (!b || !w) return fail(MCBS_EINVAL, "null argument");
    if (!arrays_set(w, 2)) return fail(MCBS_EINVAL, "mcbs_wrapper_buffers: every array but n_done and executed is required");   // (the last two members)
    mcbs_row_copies none{};
    const mcbs_row_copies* rc[2] = {keep ? keep : &none, fresh ? fresh : &none};
    for (const mcbs_row_copies* c : rc) {
        if (c->n > 8) return fail(MCBS_EINVAL, "at most eight arrays per list");
        for (uint32_t i = 0; i < c->n; ++i) if (!c->src[i] || !c->dst[i]) return fail(MCBS_EINVAL, "null array");
    }
    if (auto_reset && !b->reset_digest_ok)
        return fail(MCBS_ESTATE, "no reset observation yet: reset the whole batch (mcbs_reset, NULL mask) and observe it once before the first call");
    A->w = *w; A->modifier = modifier; A->max_timesteps = max_timesteps; A->auto_reset = auto_reset; A->pad = 0;
    A->keep = *rc[0]; A->fresh = *rc[1]; A->digest = b->digest; A->reset_digest = b->reset_digest;
    return MCBS_OK;
}

// What every attacker-turn entry point checks first, in the order the refusal tests see (finish_args, the draw tape, exactly one action
// encoding) -> the turn's StepIO, and in *finish the arguments of the wrapper-finish half where the caller launches it on its own
static int attacker_turn_io(mcbs_batch* b, const int64_t* multidiscrete, const int64_t* discrete, int32_t* decoded, const mcbs_info_buffers* info,
                            const mcbs_wrapper_buffers* w, float modifier, int32_t max_timesteps, int32_t auto_reset, const mcbs_row_copies* keep,
                            const mcbs_row_copies* fresh, StepIO* io, WrapperFinishArgs* finish = nullptr) {
    WrapperFinishArgs checked_only;
    int rc = finish_args(b, w, modifier, max_timesteps, auto_reset, keep, fresh, finish ? finish : &checked_only);
    if (rc) return rc;
    if ((rc = draws_ok(b))) return rc;
    if (!multidiscrete == !discrete) return fail(MCBS_EINVAL, "need exactly one action encoding");
    *io = make_io(b, decoded, const_cast<float*>(w->reward), const_cast<uint8_t*>(w->terminated), info);
    return MCBS_OK;
}

// ... and what it does after its one launch: every env's digest was written (or, for an intercepted action, stands); own_lists: with the
// discovery order of its own observation (the training turn)
static int turn_launched(mcbs_batch* b, const char* what, bool own_lists = false) {
    const int rc = launch_ok(what);
    if (rc) return rc;
    if (own_lists) b->digest_lists = true;
    b->digest_state = 1;
    return MCBS_OK;
}

extern "C" int mcbs_attacker_wrapper_finish(mcbs_batch* b, const mcbs_wrapper_buffers* w, float modifier, int32_t max_timesteps, int32_t auto_reset,
                                            const mcbs_row_copies* keep, const mcbs_row_copies* fresh, void* stream) {
    WrapperFinishArgs A;
    const int rc = finish_args(b, w, modifier, max_timesteps, auto_reset, keep, fresh, &A);
    if (rc) return rc;
    MCBS_ON_DEVICE(b);
    b->all_fresh = false;
    hipLaunchKernelGGL(wrapper_finish_kernel, dim3((b->S.E + 255) / 256), dim3(256), 0, (hipStream_t)stream, b->S, b->T, A);
    return launch_ok("wrapper finish");
}

extern "C" int32_t mcbs_attacker_wrapper_step_launches(const mcbs_batch* b, int32_t with_masks) {
    if (!b) return 0;
    return (!with_masks && b->variant.fused_wrapper) ? 1 : 3;
}

// The whole wrapper step in ONE launch (mcbs_wrapper_fused.hip) when the batch (variant.fused_wrapper) and the request fit it: no mask
// field, observation rows of whole 16-byte vectors, every requested field paired with its terminal array and its reset row
// (auto_reset).  fused_wrapper_args: the kernel's argument block -> true when batch and request fit (mcbs_two_agent_step shares it).
static bool fused_wrapper_args(const mcbs_batch* b, const int64_t* multidiscrete, const int64_t* discrete, int32_t* decoded, const mcbs_obs_buffers* o,
                               const mcbs_wrapper_buffers* w, float modifier, int32_t max_timesteps, int32_t auto_reset, const mcbs_row_copies* keep,
                               const mcbs_row_copies* fresh, FusedArgs* out) {
    const mcbs_topo_header* h = b->topo->H();
    const uint32_t Nm = b->cfg.maximum_node_count, Cm = b->cfg.maximum_total_credentials, K = b->cfg.maximum_discoverable_credentials_per_action;
    if (!b->variant.fused_wrapper || o->mask_local || o->mask_remote || o->mask_connect || o->mask_discrete) return false;
    const uint32_t NP = b->C.n_props;
    FusedArgs& A = *out;
    A = FusedArgs{};
    A.w = *w; A.modifier = modifier; A.max_timesteps = max_timesteps; A.auto_reset = auto_reset;
    A.Nmax = Nm; A.Cmax = Cm; A.K = K; A.NP = NP;
    A.md = multidiscrete; A.discrete = discrete; A.decoded = decoded;
    int32_t* fields[FUSED_FIELDS] = {o->scalars, o->leaked_credentials, o->credential_cache_matrix, o->discovered_nodes_properties, o->nodes_privilegelevel};
    const uint32_t dw[FUSED_FIELDS] = {7u, K * 4u, Cm * 2u, Nm * NP, Nm};
    uint32_t off = 0;
    for (uint32_t f = 0; f < FUSED_FIELDS; ++f) {
        A.obs[f] = fields[f]; A.dwords[f] = dw[f]; A.fresh_off[f] = off;
        const bool vec = f > 0 && dw[f] % 4u == 0 && !(f == 3 && NP < 4u);          // whole 16-byte vectors per env row, else dword by dword
        A.d_u4[f] = fast_div_host(vec ? dw[f] / 4u : (dw[f] ? dw[f] : 1u));
        if (!fields[f]) continue;
        if (dw[f] == 0 || (vec && reinterpret_cast<uintptr_t>(fields[f]) % 16u != 0)) return false;
        if (auto_reset) {
            int ki = -1, fi = -1;
            for (uint32_t i = 0; keep && i < keep->n; ++i) if (keep->src[i] == fields[f] && keep->row_bytes[i] == 4ull * dw[f]) ki = (int)i;
            for (uint32_t i = 0; fresh && i < fresh->n; ++i) if (fresh->dst[i] == fields[f] && fresh->row_bytes[i] == 4ull * dw[f]) fi = (int)i;
            if (ki < 0 || fi < 0) return false;
            A.term[f] = static_cast<int32_t*>(keep->dst[ki]);
            A.fresh[f] = static_cast<const int32_t*>(fresh->src[fi]);
            if (vec && reinterpret_cast<uintptr_t>(A.term[f]) % 16u != 0) return false;
        }
        off += (dw[f] + 3u) & ~3u;
    }
    if (off > FUSED_FRESH_DWORDS) return false;
    if (auto_reset) {          // every array the generic finish would copy must be one the fused kernel handles (no extra fields)
        uint32_t n_fields = 0;
        for (uint32_t f = 0; f < FUSED_FIELDS; ++f) n_fields += fields[f] ? 1u : 0u;
        if ((keep ? keep->n : 0u) != n_fields || (fresh ? fresh->n : 0u) != n_fields) return false;
    }
    A.dNP = fast_div_host(NP ? NP : 1u);
    A.digest = b->digest; A.reset_digest = b->reset_digest;
    A.triples = reinterpret_cast<const mcbs_triple*>(b->topo->dev + h->off_triple);
    A.n_triples = h->n_triples;
    return true;
}

// Returns 1 when it launched, 0 when the caller should run the three launches, < 0 on error.
static int try_fused_wrapper_step(mcbs_batch* b, const int64_t* multidiscrete, const int64_t* discrete, int32_t* decoded, const StepIO& io,
                                  const mcbs_obs_buffers* o, const mcbs_wrapper_buffers* w, float modifier, int32_t max_timesteps, int32_t auto_reset,
                                  const mcbs_row_copies* keep, const mcbs_row_copies* fresh, hipStream_t st) {
    FusedArgs A;
    if (!fused_wrapper_args(b, multidiscrete, discrete, decoded, o, w, modifier, max_timesteps, auto_reset, keep, fresh, &A)) return 0;
    b->all_fresh = false;
    const dim3 grid((b->S.E + 63u) / 64u), block(FUSED_THREADS);
    pick<MCBS_DEFENDER_SCAN_AND_REIMAGE, MCBS_DEFENDER_EXTERNAL, MCBS_DEFENDER_NONE>((int)b->cfg.defender_kind, [&](auto def) {
        hipLaunchKernelGGL((wrapper_fused_kernel<decltype(def)::value>), grid, block, 0, st, b->S, b->T, b->C_dev, io, A);
    });
    const int rc = turn_launched(b, "wrapper step (one launch)");
    return rc ? rc : 1;
}

extern "C" int mcbs_attacker_wrapper_step(mcbs_batch* b, const int64_t* multidiscrete, const int64_t* discrete, int32_t* decoded,
                                          const mcbs_info_buffers* info, const mcbs_obs_buffers* obs, const mcbs_wrapper_buffers* w, float modifier,
                                          int32_t max_timesteps, int32_t auto_reset, const mcbs_row_copies* keep, const mcbs_row_copies* fresh,
                                          void* stream) {
    if (!b || !w || !decoded || !obs) return fail(MCBS_EINVAL, "null argument");
    MCBS_ON_DEVICE(b);
    WrapperFinishArgs A;
    StepIO io;
    // (all checks before the first launch)
    int rc = attacker_turn_io(b, multidiscrete, discrete, decoded, info, w, modifier, max_timesteps, auto_reset, keep, fresh, &io, &A);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    uint8_t* invalid = const_cast<uint8_t*>(w->invalid);
    if ((rc = try_fused_wrapper_step(b, multidiscrete, discrete, decoded, io, obs, w, modifier, max_timesteps, auto_reset, keep, fresh, st)) != 0)
        return rc < 0 ? rc : MCBS_OK;
    // three launches, the step split around the observation: decode + attacker phase, observation, defender phase + wrapper finish
    // (mcbs_aux.hip), in step_kernel's launch shape
    b->all_fresh = false;
    step_variant(b, [&](auto wt, auto def) {
        hipLaunchKernelGGL((decode_step1_kernel<decltype(wt)::value, decltype(def)::value>), step_grid(b), dim3(64), step_lds(b), st, b->S, b->T, b->C_dev, io,
                           b->cfg.maximum_node_count, b->cfg.maximum_total_credentials, multidiscrete, discrete, invalid);
    });
    if ((rc = launch_ok("decode + step (attacker phase)"))) return rc;
    if ((rc = launch_obs(b, obs, st))) return rc;
    step_variant(b, [&](auto wt, auto def) {
        hipLaunchKernelGGL((step2_finish_kernel<decltype(wt)::value, decltype(def)::value>), step_grid(b), dim3(64), step_lds(b), st, b->S, b->T, b->C_dev, io, A);
    });
    return launch_ok("step (defender phase) + wrapper finish");
}

extern "C" int mcbs_defender_wrapper_post(mcbs_batch* b, const mcbs_defender_wrapper_buffers* w, const mcbs_defender_wrapper_cfg* cfg, void* stream) {
    if (!b || !w || !cfg) return fail(MCBS_EINVAL, "null argument");
    MCBS_ON_DEVICE(b);
    if (!arrays_set(w, 0)) return fail(MCBS_EINVAL, "mcbs_defender_wrapper_buffers: every array is required");
    hipLaunchKernelGGL(defender_wrapper_post_kernel, dim3((b->S.E + 255) / 256), dim3(256), 0, (hipStream_t)stream, b->S.E, *w, *cfg);
    return launch_ok("defender wrapper post");
}

extern "C" int mcbs_step_info(mcbs_batch* b, const mcbs_info_buffers* info, void* stream) {
    if (!b || !info) return fail(MCBS_EINVAL, "null argument");
    MCBS_ON_DEVICE(b);
    StepIO io = make_io(b, nullptr, nullptr, nullptr, info);
    hipLaunchKernelGGL(info_kernel, dim3((b->S.E + 255) / 256), dim3(256), 0, (hipStream_t)stream, b->S, io);
    return launch_ok("info");
}

extern "C" int mcbs_sample_actions(mcbs_batch* b, int32_t valid, uint64_t seed, uint64_t step, int32_t* actions_out, void* stream) {
    if (!b || !actions_out) return fail(MCBS_EINVAL, "null argument");
    MCBS_ON_DEVICE(b);
    hipLaunchKernelGGL(sample_kernel, dim3((b->S.E + 127) / 128), dim3(128), 0, (hipStream_t)stream, b->S, b->T, b->C_dev, (int)valid, seed, step,
                       b->cfg.maximum_node_count, b->cfg.maximum_total_credentials, actions_out);
    return launch_ok("sample");
}

extern "C" int mcbs_decode_attacker_actions(mcbs_batch* b, const int64_t* multidiscrete, const int64_t* discrete,
                                            int32_t* actions_out, uint8_t* invalid_out, void* stream) {
    if (!b || !actions_out || !invalid_out || (!multidiscrete == !discrete)) return fail(MCBS_EINVAL, "need exactly one action encoding and both outputs");
    MCBS_ON_DEVICE(b);
    hipLaunchKernelGGL(decode_kernel, dim3((b->S.E + 255) / 256), dim3(256), 0, (hipStream_t)stream, b->S, b->C_dev,
                       b->cfg.maximum_node_count, b->cfg.maximum_total_credentials, multidiscrete, discrete, actions_out, invalid_out);
    return launch_ok("decode");
}

// ------------------------------------------------------------------ action mask -> logits
extern "C" uint64_t mcbs_discrete_action_count(const mcbs_batch* b) {
    if (!b) return 0;
    const uint64_t N = b->cfg.maximum_node_count, C = b->cfg.maximum_total_credentials;
    return N * N * b->C.P * C + N * b->C.L + N * N * b->C.R;
}

// The Discrete mask of the last observation is rebuilt from the per-env digests (mcbs_mask_logits, mcbs_pack_action_mask): refused
// under ExternalRandomEvents and while the digests cannot be trusted
static int digest_usable(const mcbs_batch* b, const char* who) {
    if (b->cfg.defender_kind == MCBS_DEFENDER_RANDOM_EVENTS)
        return fail(MCBS_ESTATE, "%s: under ExternalRandomEvents a node's local-vulnerability mask changes with the defender's "
                                 "edits and is not part of the observation digest; use the materialised mask (mcbs_observe)", who);
    if (b->digest_state != 1)
        return fail(MCBS_ESTATE, b->digest_state == 0 ? "%s: no observation has been taken since the batch was created, wholly reset or given a state "
                                                        "(the mask is rebuilt from the digest the last observation left per env)"
                                                      : "%s: envs were reset by mask and not re-observed (mcbs_observe_masked) since", who);
    return MCBS_OK;
}

// A Discrete actions and W mask words per row, as every row-shaped entry point sees the batch (one launch indexes actions in 32 bits)
static int discrete_dims(const mcbs_batch* b, uint32_t& A, uint32_t& W) {
    const uint64_t A64 = mcbs_discrete_action_count(b);
    if (A64 >= (1ull << 31)) return fail(MCBS_ELIMIT, "Discrete action space too large for one launch");
    A = (uint32_t)A64; W = (A + 31u) / 32u;
    return MCBS_OK;
}

// The caller's rows hold the batch's Discrete space: `words` dwords per row of packed bits, `stride` elements per row of logits-shaped
// values, each named as the entry point's messages name it; a NULL name skips that check
static int rows_hold(uint32_t A, const char* words_name, size_t words, const char* stride_name, size_t stride) {
    const uint32_t W = (A + 31u) / 32u;
    if (words_name && words < W) return fail(MCBS_EINVAL, "%s %zu is shorter than the %u words of %u Discrete actions", words_name, words, W, A);
    if (stride_name && stride < A) return fail(MCBS_EINVAL, "%s %zu is shorter than the %u Discrete actions", stride_name, stride, A);
    return MCBS_OK;
}

static int discrete_geom(const mcbs_batch* b, LogitsGeom& G) {
    uint32_t W;
    int rc;
    if ((rc = discrete_dims(b, G.A, W))) return rc;
    G.N = b->cfg.maximum_node_count; G.C = b->cfg.maximum_total_credentials; G.L = b->C.L; G.R = b->C.R; G.RL = b->C.P * G.C;
    G.M = G.N * G.N * G.RL; G.ML = G.N * G.L;
    G.dRL = fast_div_host(G.RL); G.dC = fast_div_host(G.C); G.dN = fast_div_host(G.N); G.dL = fast_div_host(G.L); G.dR = fast_div_host(G.R);
    return MCBS_OK;
}

// One wavefront per row, four per workgroup along grid.x, at most `cap` workgroups: the kernels loop over rows beyond 4 * grid.x
// (gridDim.x * blockDim.x must stay below 2^32), so n_rows is not limited by the launch.  Very long rows split their `chunks` of 64
// pieces over grid.y.
static dim3 rows_grid(uint64_t n_rows, uint32_t cap, uint32_t chunks = 1u) {
    const uint64_t blocks = (n_rows + 3u) / 4u;
    return dim3(blocks < cap ? (uint32_t)blocks : cap, chunks < 64u ? chunks : 64u);
}

template <uint32_t N> using GroupWidth = std::integral_constant<uint32_t, N>;

// The store group of a row-writing kernel (mcbs_rowstore.h) from what the rows allow: the widest of 16, 8 and 4 bytes that both the
// base pointer and the row stride are multiples of and that holds at least MIN_GW elements, as one vector store; else groups of
// MIN_GW elements stored one by one.  launch(ES, GW, VEC) gets the element size, the group width and the vector flag as
// std::integral_constant, so each caller instantiates exactly the kernels this ladder can pick.
template <uint32_t ES, uint32_t MIN_GW, typename Launch>
static void rows_dispatch_sized(const void* base, size_t row_stride, Launch&& launch) {
    const uintptr_t p0 = reinterpret_cast<uintptr_t>(base);
    const size_t rb = row_stride * ES;
    constexpr std::integral_constant<uint32_t, ES> es{};
    if (rb % 16 == 0 && p0 % 16 == 0) return launch(es, GroupWidth<16u / ES>{}, std::true_type{});
    if constexpr (8u / ES >= MIN_GW) if (rb % 8 == 0 && p0 % 8 == 0) return launch(es, GroupWidth<8u / ES>{}, std::true_type{});      // rows only 8-byte aligned (Chain-10: 14 172 bf16 actions)
    if constexpr (4u / ES >= MIN_GW && MIN_GW > 1u) if (rb % 4 == 0 && p0 % 4 == 0) return launch(es, GroupWidth<4u / ES>{}, std::true_type{});
    launch(es, GroupWidth<MIN_GW>{}, std::bool_constant<MIN_GW == 1u>{});       // (a group of one element is its own vector store)
}
// elem_size 4 or 2 bytes; MIN_GW32 / MIN_GW16: the narrowest group of the caller's kernels for either
template <uint32_t MIN_GW32, uint32_t MIN_GW16, typename Launch>
static void rows_dispatch(size_t elem_size, const void* base, size_t row_stride, Launch&& launch) {
    if (elem_size == 4u) rows_dispatch_sized<4u, MIN_GW32>(base, row_stride, launch);
    else rows_dispatch_sized<2u, MIN_GW16>(base, row_stride, launch);
}
template <uint32_t ES> using LogitsElem = std::conditional_t<ES == 4u, float, uint16_t>;       // logits rows: fp32, or bf16 patterns
template <uint32_t ES> static LogitsElem<ES> logits_fill(float fill) { if constexpr (ES == 4u) return fill; else return (uint16_t)bf16_bits(fill); }

extern "C" int mcbs_mask_logits(mcbs_batch* b, void* logits, int32_t dtype, size_t row_stride, float fill, void* stream) {
    if (!b || !logits) return fail(MCBS_EINVAL, "null argument");
    MCBS_ON_DEVICE(b);
    if (dtype != MCBS_LOGITS_F32 && dtype != MCBS_LOGITS_BF16) return fail(MCBS_EINVAL, "logits dtype must be MCBS_LOGITS_F32 or MCBS_LOGITS_BF16");
    int rc;
    if ((rc = digest_usable(b, "mcbs_mask_logits"))) return rc;
    LogitsGeom G;
    if ((rc = discrete_geom(b, G))) return rc;
    if ((rc = rows_hold(G.A, nullptr, 0, "row_stride", row_stride))) return rc;
    hipStream_t st = (hipStream_t)stream;
    // one wavefront per env, four per workgroup; very large action spaces split their chunks of 64 spans over grid.x
    auto grid_for = [&](uint32_t gw) { const uint32_t chunks = (((G.A + gw - 1u) / gw + 15u + 63u) / 64u + 63u) / 64u;   /* spans are shifted by up to 15 groups */ return dim3(chunks < 64u ? chunks : 64u, (b->S.E + 3u) / 4u); };
    rows_dispatch<4u, 4u>(dtype == MCBS_LOGITS_F32 ? 4u : 2u, logits, row_stride, [&](auto es, auto gw, auto vec) {
        using LT = LogitsElem<decltype(es)::value>;
        constexpr uint32_t GW = decltype(gw)::value;
        pick<0, 1>((int)b->digest_lists, [&](auto own) {
            hipLaunchKernelGGL((mask_logits_kernel<LT, GW, decltype(vec)::value, decltype(own)::value != 0>), grid_for(GW), dim3(256), 0, st, b->S, b->T,
                               b->C_dev, b->digest, static_cast<LT*>(logits), row_stride, logits_fill<decltype(es)::value>(fill), G);
        });
    });
    return launch_ok("mask logits");
}

// ------------------------------------------------------------------ bit-packed action masks
extern "C" int mcbs_pack_action_mask(mcbs_batch* b, uint32_t* bits, size_t row_words, void* stream) {
    if (!b || !bits) return fail(MCBS_EINVAL, "null argument");
    MCBS_ON_DEVICE(b);
    int rc;
    if ((rc = digest_usable(b, "mcbs_pack_action_mask"))) return rc;
    LogitsGeom G;
    if ((rc = discrete_geom(b, G))) return rc;
    if ((rc = rows_hold(G.A, "row_words", row_words, nullptr, 0))) return rc;
    pick<0, 1>((int)b->digest_lists, [&](auto own) {
        hipLaunchKernelGGL((pack_mask_kernel<decltype(own)::value != 0>), dim3((b->S.E + 3u) / 4u), dim3(256), 0, (hipStream_t)stream, b->S, b->T, b->C_dev,
                           b->digest, bits, row_words, G);
    });
    return launch_ok("pack action mask");
}

extern "C" int mcbs_apply_packed_mask(const mcbs_batch* b, const uint32_t* bits, size_t bits_row_words, void* logits, int32_t dtype,
                                      size_t logits_row_stride, uint64_t n_rows, float fill, void* stream) {
    if (!b || !bits || !logits) return fail(MCBS_EINVAL, "null argument");
    MCBS_ON_DEVICE(b);
    if (dtype != MCBS_LOGITS_F32 && dtype != MCBS_LOGITS_BF16) return fail(MCBS_EINVAL, "logits dtype must be MCBS_LOGITS_F32 or MCBS_LOGITS_BF16");
    uint32_t A, W;
    int rc;
    if ((rc = discrete_dims(b, A, W))) return rc;
    if ((rc = rows_hold(A, "bits_row_words", bits_row_words, "logits_row_stride", logits_row_stride))) return rc;
    if (n_rows == 0) return MCBS_OK;
    hipStream_t st = (hipStream_t)stream;
    rows_dispatch<4u, 4u>(dtype == MCBS_LOGITS_F32 ? 4u : 2u, logits, logits_row_stride, [&](auto es, auto gw, auto vec) {
        using LT = LogitsElem<decltype(es)::value>;
        constexpr uint32_t GW = decltype(gw)::value;
        const dim3 grid = rows_grid(n_rows, 65536u, (((A + GW - 1u) / GW + 31u + 63u) / 64u + 63u) / 64u);   /* spans shifted by < 32 groups */
        hipLaunchKernelGGL((apply_packed_kernel<LT, GW, decltype(vec)::value>), grid, dim3(256), 0, st, bits, bits_row_words, static_cast<LT*>(logits),
                           logits_row_stride, n_rows, logits_fill<decltype(es)::value>(fill), A);
    });
    return launch_ok("apply packed mask");
}

extern "C" int mcbs_unpack_action_mask(const mcbs_batch* b, const uint32_t* bits, size_t bits_row_words, uint8_t* out, size_t out_row_stride,
                                       uint64_t n_rows, void* stream) {
    if (!b || !bits || !out) return fail(MCBS_EINVAL, "null argument");
    MCBS_ON_DEVICE(b);
    uint32_t A, W;
    int rc;
    if ((rc = discrete_dims(b, A, W))) return rc;
    if ((rc = rows_hold(A, "bits_row_words", bits_row_words, "out_row_stride", out_row_stride))) return rc;
    if (n_rows == 0) return MCBS_OK;
    hipLaunchKernelGGL(unpack_mask_kernel, rows_grid(n_rows, 65536u, ((A + 15u + 15u) / 16u + 63u) / 64u), dim3(256), 0, (hipStream_t)stream, bits, bits_row_words, out, out_row_stride, n_rows, A);
    return launch_ok("unpack action mask");
}

// ------------------------------------------------------------------ action-mask keys
static MaskKeyGeom mask_key_geom(const mcbs_batch* b) {
    MaskKeyGeom K;
    const uint32_t n = b->topo->H()->n_nodes;
    K.Nk = b->cfg.maximum_node_count < n ? b->cfg.maximum_node_count : n;
    K.own_words = (K.Nk + 31u) / 32u; K.node_words = (K.Nk + 3u) / 4u; K.Wk = 1u + K.own_words + K.node_words;
    K.dWk = fast_div_host(K.Wk);
    return K;
}

extern "C" uint64_t mcbs_mask_key_words(const mcbs_batch* b) { return b ? mask_key_geom(b).Wk : 0; }

extern "C" int mcbs_store_mask_keys(mcbs_batch* b, uint32_t* keys, size_t row_words, void* stream) {
    if (!b || !keys) return fail(MCBS_EINVAL, "null argument");
    MCBS_ON_DEVICE(b);
    int rc;
    if ((rc = digest_usable(b, "mcbs_store_mask_keys"))) return rc;
    const MaskKeyGeom K = mask_key_geom(b);
    if (row_words < K.Wk) return fail(MCBS_EINVAL, "row_words %zu is shorter than the %u words of a mask key", row_words, K.Wk);
    const uint64_t total = (uint64_t)b->S.E * K.Wk;                  // one thread per key word
    if (total >= (1ull << 31)) return fail(MCBS_ELIMIT, "too many envs for one launch of mcbs_store_mask_keys");
    pick<0, 1>((int)b->digest_lists, [&](auto own) {
        hipLaunchKernelGGL((store_mask_keys_kernel<decltype(own)::value != 0>), dim3((uint32_t)((total + 255u) / 256u)), dim3(256), 0, (hipStream_t)stream,
                           b->S, b->digest, keys, row_words, K, (uint32_t)total);
    });
    return launch_ok("store mask keys");
}

extern "C" int mcbs_expand_mask_keys(const mcbs_batch* b, const uint32_t* keys, size_t key_row_words, const int64_t* index, uint64_t n_source_rows,
                                     uint32_t* bits, size_t bits_row_words, uint64_t n_rows, void* stream) {
    if (!b || !keys || !bits) return fail(MCBS_EINVAL, "null argument");
    MCBS_ON_DEVICE(b);
    LogitsGeom G;
    int rc;
    if ((rc = discrete_geom(b, G))) return rc;
    if ((rc = rows_hold(G.A, "bits_row_words", bits_row_words, nullptr, 0))) return rc;
    const MaskKeyGeom K = mask_key_geom(b);
    if (key_row_words < K.Wk) return fail(MCBS_EINVAL, "key_row_words %zu is shorter than the %u words of a mask key", key_row_words, K.Wk);
    if (!index && n_rows > n_source_rows) return fail(MCBS_EINVAL, "mcbs_expand_mask_keys: %llu rows asked of %llu stored ones and no index",
                                                      (unsigned long long)n_rows, (unsigned long long)n_source_rows);
    if (n_rows == 0) return MCBS_OK;
    hipLaunchKernelGGL(expand_mask_keys_kernel, rows_grid(n_rows, 65536u), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const mcbs_node_static*>(b->T.base + b->C.off_node), b->topo->H()->n_nodes, K, G, keys, key_row_words, index,
                       n_source_rows, bits, bits_row_words, n_rows);
    return launch_ok("expand mask keys");
}

// ------------------------------------------------------------------ masked categorical head
// arguments common to the two forms; `who` names the entry point in messages
static int categorical_args(const char* who, const void* logits, int32_t dtype, size_t row_stride, int32_t mode, const int64_t* actions,
                            const float* log_prob, uint32_t A) {
    if (logits && dtype != MCBS_LOGITS_F32 && dtype != MCBS_LOGITS_BF16) return fail(MCBS_EINVAL, "%s: logits dtype must be MCBS_LOGITS_F32 or MCBS_LOGITS_BF16", who);
    if (mode != MCBS_CATEGORICAL_SAMPLE && mode != MCBS_CATEGORICAL_ARGMAX && mode != MCBS_CATEGORICAL_EVALUATE)
        return fail(MCBS_EINVAL, "%s: mode must be MCBS_CATEGORICAL_SAMPLE, _ARGMAX or _EVALUATE", who);
    if (!actions || !log_prob) return fail(MCBS_EINVAL, "%s: actions and log_prob must not be NULL", who);
    return logits ? rows_hold(A, nullptr, 0, (std::string(who) + ": row_stride").c_str(), row_stride) : MCBS_OK;
}

static void categorical_launch(const mcbs_batch* b, bool live, const LogitsGeom& G, const uint32_t* bits, size_t bits_row_words, int32_t dtype,
                               const CatIO& io, hipStream_t st) {
    const dim3 grid = rows_grid(io.n_rows, 65536u), block(256);
    pick<2, 4>(dtype == MCBS_LOGITS_BF16 && io.logits ? 2 : 4, [&](auto es) {       // element size: bf16 patterns, else fp32 (also without logits)
        pick<2, 1, 0>(live ? (b->digest_lists ? 2 : 1) : 0, [&](auto lv) {          // 2: live, digests with a discovery order of their own
            hipLaunchKernelGGL((masked_categorical_kernel<LogitsElem<(uint32_t)decltype(es)::value>, decltype(lv)::value != 0, decltype(lv)::value == 2>),
                               grid, block, 0, st, b->S, b->T, b->C_dev, b->digest, G, bits, bits_row_words, io);
        });
    });
}

extern "C" int mcbs_masked_categorical(mcbs_batch* b, const void* logits, int32_t dtype, size_t row_stride, int32_t mode, int64_t* actions,
                                       float* log_prob, float* entropy, uint32_t* n_allowed, const float* uniforms, uint64_t seed, uint64_t step,
                                       uint32_t* bad_actions, void* stream) {
    if (!b) return fail(MCBS_EINVAL, "null argument");
    MCBS_ON_DEVICE(b);
    int rc;
    if ((rc = digest_usable(b, "mcbs_masked_categorical"))) return rc;
    LogitsGeom G;
    if ((rc = discrete_geom(b, G))) return rc;
    if ((rc = categorical_args("mcbs_masked_categorical", logits, dtype, row_stride, mode, actions, log_prob, G.A))) return rc;
    CatIO io{logits, row_stride, actions, log_prob, entropy, n_allowed, uniforms, bad_actions, seed, step, b->cfg.env_id_base, b->S.E, (uint32_t)mode, G.A};
    categorical_launch(b, true, G, nullptr, 0, dtype, io, (hipStream_t)stream);
    return launch_ok("masked categorical");
}

extern "C" int mcbs_masked_categorical_packed(const mcbs_batch* b, const uint32_t* bits, size_t bits_row_words, uint64_t n_rows, const void* logits,
                                              int32_t dtype, size_t row_stride, int32_t mode, int64_t* actions, float* log_prob, float* entropy,
                                              uint32_t* n_allowed, const float* uniforms, uint64_t seed, uint64_t step, uint32_t* bad_actions,
                                              void* stream) {
    if (!b) return fail(MCBS_EINVAL, "null argument");
    MCBS_ON_DEVICE(b);
    int rc;
    LogitsGeom G;
    if ((rc = discrete_geom(b, G))) return rc;
    if (n_rows == 0) return MCBS_OK;
    if (!bits) return fail(MCBS_EINVAL, "mcbs_masked_categorical_packed: bits must not be NULL");
    if ((rc = rows_hold(G.A, "bits_row_words", bits_row_words, nullptr, 0))) return rc;
    if ((rc = categorical_args("mcbs_masked_categorical_packed", logits, dtype, row_stride, mode, actions, log_prob, G.A))) return rc;
    CatIO io{logits, row_stride, actions, log_prob, entropy, n_allowed, uniforms, bad_actions, seed, step, 0ull, n_rows, (uint32_t)mode, G.A};
    categorical_launch(b, false, G, bits, bits_row_words, dtype, io, (hipStream_t)stream);
    return launch_ok("masked categorical (packed)");
}

// ------------------------------------------------------------------ masked action head from the latent
static int linear_categorical_args(const char* who, const void* latent, size_t latent_row_stride, const void* weight, size_t weight_row_stride,
                                   uint32_t H, int32_t dtype, int32_t mode, const int64_t* actions, const float* log_prob) {
    if (!latent || !weight) return fail(MCBS_EINVAL, "%s: latent and weight must not be NULL (the uniform law is mcbs_masked_categorical's logits == NULL)", who);
    if (H < 1u || H > MCBS_LINEAR_MAX_H) return fail(MCBS_EINVAL, "%s: H %u: from 1 to %u", who, H, (uint32_t)MCBS_LINEAR_MAX_H);
    if (latent_row_stride < H) return fail(MCBS_EINVAL, "%s: latent_row_stride %zu is shorter than H = %u", who, latent_row_stride, H);
    if (weight_row_stride < H) return fail(MCBS_EINVAL, "%s: weight_row_stride %zu is shorter than H = %u", who, weight_row_stride, H);
    if (dtype != MCBS_LOGITS_F32 && dtype != MCBS_LOGITS_BF16) return fail(MCBS_EINVAL, "%s: dtype must be MCBS_LOGITS_F32 or MCBS_LOGITS_BF16", who);
    return categorical_args(who, nullptr, dtype, 0, mode, actions, log_prob, 0u);
}

static void linear_categorical_launch(const mcbs_batch* b, bool live, const LogitsGeom& G, const uint32_t* bits, size_t bits_row_words, int32_t dtype,
                                      const LinIO& lin, const CatIO& io, hipStream_t st) {
    const dim3 grid = rows_grid(io.n_rows, 65536u), block(256);
    pick<2, 4>(dtype == MCBS_LOGITS_BF16 ? 2 : 4, [&](auto es) {
        pick<2, 1, 0>(live ? (b->digest_lists ? 2 : 1) : 0, [&](auto lv) {
            hipLaunchKernelGGL((masked_linear_categorical_kernel<LogitsElem<(uint32_t)decltype(es)::value>, decltype(lv)::value != 0, decltype(lv)::value == 2>),
                               grid, block, 0, st, b->S, b->T, b->C_dev, b->digest, G, bits, bits_row_words, lin, io);
        });
    });
}

extern "C" int mcbs_masked_linear_categorical(mcbs_batch* b, const void* latent, size_t latent_row_stride, const void* weight, size_t weight_row_stride,
                                              const void* bias, uint32_t H, int32_t dtype, int32_t mode, int64_t* actions, float* log_prob,
                                              float* entropy, uint32_t* n_allowed, const float* uniforms, uint64_t seed, uint64_t step,
                                              uint32_t* bad_actions, void* stream) {
    if (!b) return fail(MCBS_EINVAL, "null argument");
    MCBS_ON_DEVICE(b);
    int rc;
    if ((rc = digest_usable(b, "mcbs_masked_linear_categorical"))) return rc;
    LogitsGeom G;
    if ((rc = discrete_geom(b, G))) return rc;
    if ((rc = linear_categorical_args("mcbs_masked_linear_categorical", latent, latent_row_stride, weight, weight_row_stride, H, dtype, mode, actions, log_prob)))
        return rc;
    const LinIO lin{latent, weight, bias, latent_row_stride, weight_row_stride, H};
    CatIO io{nullptr, 0, actions, log_prob, entropy, n_allowed, uniforms, bad_actions, seed, step, b->cfg.env_id_base, b->S.E, (uint32_t)mode, G.A};
    linear_categorical_launch(b, true, G, nullptr, 0, dtype, lin, io, (hipStream_t)stream);
    return launch_ok("masked action head from the latent");
}

extern "C" int mcbs_masked_linear_categorical_packed(const mcbs_batch* b, const uint32_t* bits, size_t bits_row_words, uint64_t n_rows, const void* latent,
                                                     size_t latent_row_stride, const void* weight, size_t weight_row_stride, const void* bias, uint32_t H,
                                                     int32_t dtype, int32_t mode, int64_t* actions, float* log_prob, float* entropy, uint32_t* n_allowed,
                                                     const float* uniforms, uint64_t seed, uint64_t step, uint32_t* bad_actions, void* stream) {
    if (!b) return fail(MCBS_EINVAL, "null argument");
    MCBS_ON_DEVICE(b);
    int rc;
    LogitsGeom G;
    if ((rc = discrete_geom(b, G))) return rc;
    if (n_rows == 0) return MCBS_OK;
    if (!bits) return fail(MCBS_EINVAL, "mcbs_masked_linear_categorical_packed: bits must not be NULL");
    if ((rc = rows_hold(G.A, "bits_row_words", bits_row_words, nullptr, 0))) return rc;
    if ((rc = linear_categorical_args("mcbs_masked_linear_categorical_packed", latent, latent_row_stride, weight, weight_row_stride, H, dtype, mode, actions,
                                      log_prob)))
        return rc;
    const LinIO lin{latent, weight, bias, latent_row_stride, weight_row_stride, H};
    CatIO io{nullptr, 0, actions, log_prob, entropy, n_allowed, uniforms, bad_actions, seed, step, 0ull, n_rows, (uint32_t)mode, G.A};
    linear_categorical_launch(b, false, G, bits, bits_row_words, dtype, lin, io, (hipStream_t)stream);
    return launch_ok("masked action head from the latent (packed)");
}

// do rows [p, p + k * stride + A) and [q, q + k * qstride + A) (k < n, bytes) share a byte?  Exact for equal strides (rows interleaved in one
// buffer are fine), conservative otherwise: then any intersection of the two extents counts
// q_row_bytes: the width of q's rows where it differs from row_bytes, that of p's (0: the same)
static bool rows_overlap(uintptr_t p, size_t stride, uintptr_t q, size_t qstride, uint64_t n, size_t row_bytes, size_t q_row_bytes = 0) {
    if (!q_row_bytes) q_row_bytes = row_bytes;
    const uintptr_t pe = p + (uintptr_t)((n - 1u) * stride + row_bytes), qe = q + (uintptr_t)((n - 1u) * qstride + q_row_bytes);
    if (pe <= q || qe <= p) return false;
    if (stride != qstride || n == 1u) return true;
    const size_t r = (size_t)((q >= p ? q - p : stride - (p - q) % stride) % stride);       // q's rows lie r bytes behind p's, modulo the stride
    return r < row_bytes || stride - r < q_row_bytes;
}

extern "C" int mcbs_masked_categorical_grad(const mcbs_batch* b, const uint32_t* bits, size_t bits_row_words, uint64_t n_rows, const void* logits,
                                            int32_t dtype, size_t row_stride, const int64_t* actions, const float* grad_log_prob,
                                            const float* grad_entropy, void* grad_logits, size_t grad_row_stride, void* stream) {
    if (!b) return fail(MCBS_EINVAL, "null argument");
    MCBS_ON_DEVICE(b);
    int rc;
    LogitsGeom G;
    if ((rc = discrete_geom(b, G))) return rc;
    const uint32_t A = G.A;
    if (n_rows == 0) return MCBS_OK;
    if (!bits || !logits || !actions || !grad_logits)
        return fail(MCBS_EINVAL, "mcbs_masked_categorical_grad: bits, logits, actions and grad_logits must not be NULL (the uniform law has no gradient)");
    if (dtype != MCBS_LOGITS_F32 && dtype != MCBS_LOGITS_BF16) return fail(MCBS_EINVAL, "mcbs_masked_categorical_grad: logits dtype must be MCBS_LOGITS_F32 or MCBS_LOGITS_BF16");
    if ((rc = rows_hold(A, "bits_row_words", bits_row_words, "mcbs_masked_categorical_grad: row_stride", row_stride))) return rc;
    if ((rc = rows_hold(A, nullptr, 0, "mcbs_masked_categorical_grad: grad_row_stride", grad_row_stride))) return rc;
    const size_t es = dtype == MCBS_LOGITS_F32 ? 4u : 2u;
    const uintptr_t lp = reinterpret_cast<uintptr_t>(logits), gp = reinterpret_cast<uintptr_t>(grad_logits);
    if (rows_overlap(lp, row_stride * es, gp, grad_row_stride * es, n_rows, (size_t)A * es))
        return fail(MCBS_EINVAL, "mcbs_masked_categorical_grad: the grad_logits rows overlap the logits rows");
    hipStream_t st = (hipStream_t)stream;
    CatGradIO io{logits, row_stride, actions, grad_log_prob, grad_entropy, grad_logits, grad_row_stride, n_rows, A, 0u};
    rows_dispatch<4u, 4u>(es, grad_logits, grad_row_stride, [&](auto esc, auto gw, auto vec) {
        using LT = LogitsElem<decltype(esc)::value>;
        constexpr size_t gb = decltype(gw)::value * sizeof(LT);
        io.logits_vec = decltype(vec)::value && lp % gb == 0 && (row_stride * es) % gb == 0;     // the logits rows are aligned like the gradient's
        hipLaunchKernelGGL((masked_categorical_grad_kernel<LT, decltype(gw)::value, decltype(vec)::value>), rows_grid(n_rows, 65536u), dim3(256), 0, st,
                           bits, bits_row_words, io);
    });
    return launch_ok("masked categorical gradient");
}

// ------------------------------------------------------------------ masked action head from the latent: gradient
// the workspace: [n] CatGradRow, then (from a 256-byte boundary) the block partials of grad_weight [n_blocks][32 W][H] and grad_bias [n_blocks][32 W]
struct LinGradWorkspace {
    uint64_t n_blocks;
    size_t part_w, part_b, bytes;      // byte offsets and the total
};
static LinGradWorkspace linear_grad_workspace(uint32_t A, uint64_t n_rows, uint32_t H) {
    LinGradWorkspace ws{};
    if (!n_rows) return ws;
    ws.n_blocks = (n_rows + MCBS_LINEAR_GRAD_ROW_BLOCK - 1u) / MCBS_LINEAR_GRAD_ROW_BLOCK;
    const size_t per_block = (size_t)((A + 31u) / 32u) * 32u;
    ws.part_w = ((size_t)n_rows * sizeof(CatGradRow) + 255u) & ~(size_t)255u;
    ws.part_b = ws.part_w + (size_t)ws.n_blocks * per_block * H * sizeof(float);
    ws.bytes = ws.part_b + (size_t)ws.n_blocks * per_block * sizeof(float);
    return ws;
}

extern "C" size_t mcbs_masked_linear_categorical_grad_workspace(const mcbs_batch* b, uint64_t n_rows, uint32_t H) {
    uint32_t A, W;
    if (!b || discrete_dims(b, A, W) || H < 1u || H > MCBS_LINEAR_MAX_H) return 0;
    return linear_grad_workspace(A, n_rows, H).bytes;
}

extern "C" int mcbs_masked_linear_categorical_grad(const mcbs_batch* b, const uint32_t* bits, size_t bits_row_words, uint64_t n_rows, const void* latent,
                                                   size_t latent_row_stride, const void* weight, size_t weight_row_stride, const void* bias, uint32_t H,
                                                   int32_t dtype, const int64_t* actions, const float* grad_log_prob, const float* grad_entropy,
                                                   float* grad_latent, size_t grad_latent_row_stride, float* grad_weight, size_t grad_weight_row_stride,
                                                   float* grad_bias, void* workspace, size_t workspace_bytes, void* stream) {
    static const char* who = "mcbs_masked_linear_categorical_grad";
    if (!b) return fail(MCBS_EINVAL, "null argument");
    MCBS_ON_DEVICE(b);
    int rc;
    LogitsGeom G;
    if ((rc = discrete_geom(b, G))) return rc;
    const uint32_t A = G.A, W = (A + 31u) / 32u;
    if (!grad_latent && !grad_weight && !grad_bias) return fail(MCBS_EINVAL, "%s: grad_latent, grad_weight and grad_bias are all NULL", who);
    if (H < 1u || H > MCBS_LINEAR_MAX_H) return fail(MCBS_EINVAL, "%s: H %u: from 1 to %u", who, H, (uint32_t)MCBS_LINEAR_MAX_H);
    if (dtype != MCBS_LOGITS_F32 && dtype != MCBS_LOGITS_BF16) return fail(MCBS_EINVAL, "%s: dtype must be MCBS_LOGITS_F32 or MCBS_LOGITS_BF16", who);
    if (grad_latent && grad_latent_row_stride < H) return fail(MCBS_EINVAL, "%s: grad_latent_row_stride %zu is shorter than H = %u", who, grad_latent_row_stride, H);
    if (grad_weight && grad_weight_row_stride < H) return fail(MCBS_EINVAL, "%s: grad_weight_row_stride %zu is shorter than H = %u", who, grad_weight_row_stride, H);
    const bool action_pass = grad_weight || grad_bias;
    hipStream_t st = (hipStream_t)stream;
    if (n_rows) {
        if (!bits || !latent || !weight || !actions) return fail(MCBS_EINVAL, "%s: bits, latent, weight and actions must not be NULL", who);
        if (latent_row_stride < H) return fail(MCBS_EINVAL, "%s: latent_row_stride %zu is shorter than H = %u", who, latent_row_stride, H);
        if (weight_row_stride < H) return fail(MCBS_EINVAL, "%s: weight_row_stride %zu is shorter than H = %u", who, weight_row_stride, H);
        if ((rc = rows_hold(A, "bits_row_words", bits_row_words, nullptr, 0))) return rc;
    }
    const LinGradWorkspace ws = linear_grad_workspace(A, n_rows, H);
    if (ws.bytes && (!workspace || workspace_bytes < ws.bytes))
        return fail(MCBS_EINVAL, "%s: the workspace must hold %zu bytes (mcbs_masked_linear_categorical_grad_workspace), got %zu at %p", who, ws.bytes,
                    workspace_bytes, workspace);

    // no output may share a byte with an input, the workspace or another output
    const size_t es = dtype == MCBS_LOGITS_F32 ? 4u : 2u;
    Extents ext;
    ext.rows("grad_latent", grad_latent, n_rows, grad_latent_row_stride, H, 4u, true);
    ext.rows("grad_weight", grad_weight, A, grad_weight_row_stride, H, 4u, true);
    ext.bytes("grad_bias", grad_bias, (uint64_t)A * 4u, true);
    ext.bytes("workspace", workspace, ws.bytes, true);
    ext.rows("bits", bits, n_rows, bits_row_words, W, 4u, false);
    ext.rows("latent", latent, n_rows, latent_row_stride, H, es, false);
    ext.rows("weight", weight, n_rows ? A : 0u, weight_row_stride, H, es, false);
    ext.bytes("bias", bias, n_rows ? (uint64_t)A * es : 0u, false);
    ext.bytes("actions", actions, n_rows * 8u, false);
    ext.bytes("grad_log_prob", grad_log_prob, n_rows * 4u, false);
    ext.bytes("grad_entropy", grad_entropy, n_rows * 4u, false);
    if ((rc = disjoint(who, ext))) return rc;

    char* wsp = static_cast<char*>(workspace);
    LinGradIO io{actions, grad_log_prob, grad_entropy, grad_latent, grad_latent_row_stride, grad_weight, grad_weight_row_stride, grad_bias,
                 action_pass && n_rows ? reinterpret_cast<CatGradRow*>(wsp) : nullptr,
                 n_rows ? reinterpret_cast<float*>(wsp + ws.part_w) : nullptr, n_rows ? reinterpret_cast<float*>(wsp + ws.part_b) : nullptr,
                 n_rows, A, (uint32_t)ws.n_blocks};
    const LinIO lin{latent, weight, bias, latent_row_stride, weight_row_stride, H};
    if (ws.n_blocks > 0xFFFFFFFFull) return fail(MCBS_EINVAL, "%s: too many rows", who);
    if (n_rows) {
        pick<2, 4>((int)es, [&](auto esc) {
            using WT = LogitsElem<(uint32_t)decltype(esc)::value>;
            hipLaunchKernelGGL((masked_linear_categorical_grad_row_kernel<WT>), rows_grid(n_rows, 65536u), dim3(256), 0, st, bits, bits_row_words, lin, io);
            if (!action_pass) return;
            const dim3 grid((W + LIN_GRAD_WORDS - 1u) / LIN_GRAD_WORDS, ws.n_blocks < 65535u ? (uint32_t)ws.n_blocks : 65535u);
            pick<1, 2, 4, 8>(H <= 64u ? 1 : H <= 128u ? 2 : H <= 256u ? 4 : 8, [&](auto nh) {
                hipLaunchKernelGGL((masked_linear_categorical_grad_action_kernel<WT, (uint32_t)decltype(nh)::value>), grid, dim3(256), 0, st, bits,
                                   bits_row_words, lin, io);
            });
        });
    }
    if (action_pass) {
        const uint32_t blocks = (A + 3u) / 4u;
        hipLaunchKernelGGL(masked_linear_categorical_grad_reduce_kernel, dim3(blocks < 65536u ? blocks : 65536u), dim3(256), 0, st, io, H);
    }
    return launch_ok("masked action head gradient");
}

// ------------------------------------------------------------------ MultiDiscrete head
// nvec (host) -> the kernels' geometry; `who` names the entry point in messages
static int multicategorical_geom(const char* who, const uint32_t* nvec, uint32_t n_dims, McGeom& G) {
    if (!nvec) return fail(MCBS_EINVAL, "%s: nvec must not be NULL", who);
    if (n_dims < 1u || n_dims > MCBS_MAX_ACTION_DIMS) return fail(MCBS_EINVAL, "%s: n_dims %u lies outside [1, %u]", who, n_dims, (unsigned)MCBS_MAX_ACTION_DIMS);
    G = McGeom{};
    uint32_t A = 0u;
    for (uint32_t d = 0; d < n_dims; ++d) {
        if (nvec[d] < 1u || nvec[d] > 65536u) return fail(MCBS_EINVAL, "%s: nvec[%u] = %u lies outside [1, 65536]", who, d, nvec[d]);
        G.nvec[d] = nvec[d];
        G.off[d] = A;
        A += nvec[d];
    }
    G.D = n_dims;
    G.A = A;
    G.R = MC_LANES / n_dims;
    return MCBS_OK;
}

// rows per workgroup pass of the staged path (0: the rows are too wide for it)
static uint32_t multicategorical_staged_rows(const McGeom& G) {
    const uint32_t fit = MC_LDS_FLOATS / G.A;
    return fit < G.R ? fit : G.R;
}

template <class F>
static void multicategorical_dispatch(McGeom& G, bool have_logits, int32_t dtype, uint64_t n_rows, F&& launch) {
    const uint32_t staged = have_logits ? multicategorical_staged_rows(G) : 0u;
    if (staged) G.R = staged;
    const uint64_t groups = (n_rows + G.R - 1u) / G.R;
    const dim3 grid(groups < 8192u ? (uint32_t)groups : 8192u), block(MC_LANES);
    const size_t lds = (MC_LDS_HEAD + (staged ? (size_t)((G.R * G.A + 3u) & ~3u) : 0u)) * sizeof(float);
    pick<2, 4>(dtype == MCBS_LOGITS_BF16 && have_logits ? 2 : 4, [&](auto es) {          // element size: bf16 patterns, else fp32 (also without logits)
        pick<1, 0>(staged ? 1 : 0, [&](auto sg) { launch(es, sg, grid, block, lds); });
    });
}

extern "C" int mcbs_multicategorical(const mcbs_batch* b, const uint32_t* nvec, uint32_t n_dims, uint64_t n_rows, const void* logits, int32_t dtype,
                                     size_t row_stride, int32_t mode, int64_t* actions, float* log_prob, float* entropy, const float* uniforms,
                                     uint64_t seed, uint64_t step, uint64_t row_key_base, uint32_t* bad_actions, void* stream) {
    if (!b) return fail(MCBS_EINVAL, "mcbs_multicategorical: batch must not be NULL");
    MCBS_ON_DEVICE(b);
    int rc;
    McGeom G;
    if ((rc = multicategorical_geom("mcbs_multicategorical", nvec, n_dims, G))) return rc;
    if (mode != MCBS_CATEGORICAL_SAMPLE && mode != MCBS_CATEGORICAL_ARGMAX && mode != MCBS_CATEGORICAL_EVALUATE)
        return fail(MCBS_EINVAL, "mcbs_multicategorical: mode must be MCBS_CATEGORICAL_SAMPLE, _ARGMAX or _EVALUATE");
    if (step >= (1ull << 48)) return fail(MCBS_EINVAL, "mcbs_multicategorical: step %llu: at most 2^48 - 1", (unsigned long long)step);
    if (logits && dtype != MCBS_LOGITS_F32 && dtype != MCBS_LOGITS_BF16)
        return fail(MCBS_EINVAL, "mcbs_multicategorical: logits dtype must be MCBS_LOGITS_F32 or MCBS_LOGITS_BF16");
    if (logits && row_stride < G.A) return fail(MCBS_EINVAL, "mcbs_multicategorical: row_stride %zu is shorter than the %u logits of a row", row_stride, G.A);
    if (n_rows == 0) return MCBS_OK;
    if (!actions || !log_prob) return fail(MCBS_EINVAL, "mcbs_multicategorical: actions and log_prob must not be NULL");
    McIO io{logits, row_stride, actions, log_prob, entropy, uniforms, bad_actions, seed, step, row_key_base, n_rows, (uint32_t)mode};
    hipStream_t st = (hipStream_t)stream;
    multicategorical_dispatch(G, logits != nullptr, dtype, n_rows, [&](auto es, auto sg, dim3 grid, dim3 block, size_t lds) {
        hipLaunchKernelGGL((multicategorical_kernel<LogitsElem<(uint32_t)decltype(es)::value>, decltype(sg)::value != 0>), grid, block, lds, st, G, io);
    });
    return launch_ok("multicategorical");
}

extern "C" int mcbs_multicategorical_grad(const mcbs_batch* b, const uint32_t* nvec, uint32_t n_dims, uint64_t n_rows, const void* logits, int32_t dtype,
                                          size_t row_stride, const int64_t* actions, const float* grad_log_prob, const float* grad_entropy,
                                          void* grad_logits, size_t grad_row_stride, void* stream) {
    if (!b) return fail(MCBS_EINVAL, "mcbs_multicategorical_grad: batch must not be NULL");
    MCBS_ON_DEVICE(b);
    int rc;
    McGeom G;
    if ((rc = multicategorical_geom("mcbs_multicategorical_grad", nvec, n_dims, G))) return rc;
    if (dtype != MCBS_LOGITS_F32 && dtype != MCBS_LOGITS_BF16)
        return fail(MCBS_EINVAL, "mcbs_multicategorical_grad: logits dtype must be MCBS_LOGITS_F32 or MCBS_LOGITS_BF16");
    if (row_stride < G.A) return fail(MCBS_EINVAL, "mcbs_multicategorical_grad: row_stride %zu is shorter than the %u logits of a row", row_stride, G.A);
    if (grad_row_stride < G.A)
        return fail(MCBS_EINVAL, "mcbs_multicategorical_grad: grad_row_stride %zu is shorter than the %u logits of a row", grad_row_stride, G.A);
    if (n_rows == 0) return MCBS_OK;
    if (!logits || !actions || !grad_logits)
        return fail(MCBS_EINVAL, "mcbs_multicategorical_grad: logits, actions and grad_logits must not be NULL (the uniform law has no gradient)");
    const size_t es = dtype == MCBS_LOGITS_F32 ? 4u : 2u;
    if (rows_overlap(reinterpret_cast<uintptr_t>(logits), row_stride * es, reinterpret_cast<uintptr_t>(grad_logits), grad_row_stride * es, n_rows,
                     (size_t)G.A * es))
        return fail(MCBS_EINVAL, "mcbs_multicategorical_grad: the grad_logits rows overlap the logits rows");
    McGradIO io{logits, row_stride, actions, grad_log_prob, grad_entropy, grad_logits, grad_row_stride, n_rows};
    hipStream_t st = (hipStream_t)stream;
    multicategorical_dispatch(G, true, dtype, n_rows, [&](auto esc, auto sg, dim3 grid, dim3 block, size_t lds) {
        hipLaunchKernelGGL((multicategorical_grad_kernel<LogitsElem<(uint32_t)decltype(esc)::value>, decltype(sg)::value != 0>), grid, block, lds, st, G, io);
    });
    return launch_ok("multicategorical gradient");
}

// ------------------------------------------------------------------ generalized advantage estimation
extern "C" int mcbs_gae(const mcbs_batch* b, const mcbs_gae_io* io, void* stream) {
    if (!b || !io) return fail(MCBS_EINVAL, "mcbs_gae: null argument (batch or io)");
    MCBS_ON_DEVICE(b);
    const uint64_t T = io->n_steps, E = io->n_envs;
    if (T == 0 || E == 0) return MCBS_OK;
    const struct { const void* p; const char* name; } required[] = {
        {io->rewards, "rewards"}, {io->values, "values"}, {io->episode_starts, "episode_starts"}, {io->last_values, "last_values"},
        {io->last_dones, "last_dones"}, {io->advantages, "advantages"}};
    for (const auto& a : required)
        if (!a.p) return fail(MCBS_EINVAL, "mcbs_gae: %s must not be NULL", a.name);
    if (E >= (1ull << 37)) return fail(MCBS_ELIMIT, "mcbs_gae: n_envs %llu: at most 2^37 - 1", (unsigned long long)E);
    // every [T, E] array: base, row stride in elements, element size; inputs first
    struct Arr { const void* p; size_t stride; size_t es; const char* name; };
    const Arr in[] = {{io->rewards, io->rewards_stride, 4u, "rewards"}, {io->values, io->values_stride, 4u, "values"},
                      {io->episode_starts, io->episode_starts_stride, 1u, "episode_starts"}, {io->bootstrap, io->bootstrap_stride, 4u, "bootstrap"}};
    const Arr out[] = {{io->advantages, io->advantages_stride, 4u, "advantages"}, {io->returns, io->returns_stride, 4u, "returns"}};
    for (const Arr& a : in)
        if (a.p && a.stride < E) return fail(MCBS_EINVAL, "mcbs_gae: %s_stride %zu is below n_envs %llu", a.name, a.stride, (unsigned long long)E);
    for (const Arr& a : out)
        if (a.p && a.stride < E) return fail(MCBS_EINVAL, "mcbs_gae: %s_stride %zu is below n_envs %llu", a.name, a.stride, (unsigned long long)E);
    if (!std::isfinite(io->gamma) || io->gamma < 0.0 || io->gamma > 1.0) return fail(MCBS_EINVAL, "mcbs_gae: gamma %g must lie in [0, 1]", io->gamma);
    if (!std::isfinite(io->gae_lambda) || io->gae_lambda < 0.0 || io->gae_lambda > 1.0)
        return fail(MCBS_EINVAL, "mcbs_gae: gae_lambda %g must lie in [0, 1]", io->gae_lambda);
    auto addr = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
    for (const Arr& o : out) {
        if (!o.p) continue;
        for (const Arr& a : in)
            if (a.p && rows_overlap(addr(o.p), o.stride * 4u, addr(a.p), a.stride * a.es, T, (size_t)E * 4u, (size_t)E * a.es))
                return fail(MCBS_EINVAL, "mcbs_gae: the %s rows overlap the %s rows", o.name, a.name);
        // the two [E] rows: any intersection with the output's extent counts (a stride of their own, 0, never equals the output's)
        if (rows_overlap(addr(o.p), o.stride * 4u, addr(io->last_values), 0u, T, (size_t)E * 4u))
            return fail(MCBS_EINVAL, "mcbs_gae: the %s rows overlap last_values", o.name);
        if (rows_overlap(addr(o.p), o.stride * 4u, addr(io->last_dones), 0u, T, (size_t)E * 4u, (size_t)E))
            return fail(MCBS_EINVAL, "mcbs_gae: the %s rows overlap last_dones", o.name);
    }
    if (io->returns && rows_overlap(addr(io->advantages), io->advantages_stride * 4u, addr(io->returns), io->returns_stride * 4u, T, (size_t)E * 4u))
        return fail(MCBS_EINVAL, "mcbs_gae: the advantages rows overlap the returns rows");
    GaeIO k{io->rewards, io->values, io->episode_starts, io->bootstrap, io->last_values, io->last_dones, io->advantages, io->returns, T, E,
            io->rewards_stride, io->values_stride, io->episode_starts_stride, io->bootstrap_stride, io->advantages_stride, io->returns_stride,
            (float)io->gamma, (float)(io->gamma * io->gae_lambda)};
    const dim3 grid((uint32_t)((E + 63u) / 64u)), block(64);
    hipStream_t st = (hipStream_t)stream;
    constexpr uint32_t U = MCBS_GAE_U;
    pick<1, 0>(io->bootstrap != nullptr, [&](auto boot) {
        pick<1, 0>(io->returns != nullptr, [&](auto ret) {
            hipLaunchKernelGGL((gae_kernel<U, decltype(boot)::value != 0, decltype(ret)::value != 0>), grid, block, 0, st, k);
        });
    });
    return launch_ok("gae");
}

// ------------------------------------------------------------------ feature encoder
struct mcbs_feature_layout {
    int32_t device = 0;
    FeatGeom G{};
    uint32_t* desc_dev = nullptr;
    uint2* elems_dev = nullptr;     // per source value: (first one-hot column, classes) of its element; NULL when two elements share a value
    FlElem* order_dev = nullptr;    // per element in row order: (first one-hot column, classes, source value): what the first-layer calls walk
    uint32_t fields_used = 0;       // bit k: some descriptor reads observation field k
    uint64_t A = 0;                 // Discrete actions of the batch the layout was made for
    uint32_t n_elements = 0;        // one-hot elements of a row
    std::vector<uint32_t> src_classes;      // per source value: the largest class count of an element that reads it (0: none does)
};

extern "C" int mcbs_feature_layout_create(const mcbs_batch* b, const uint32_t* desc, size_t n_desc, const uint32_t* mask_ranges,
                                          size_t n_mask_ranges, mcbs_feature_layout** out) {
    if (!b || !out || (!desc && n_desc) || (!mask_ranges && n_mask_ranges)) return fail(MCBS_EINVAL, "null argument");
    if (n_mask_ranges > FEAT_MAX_RANGES) return fail(MCBS_EINVAL, "at most %u mask ranges, got %zu", FEAT_MAX_RANGES, n_mask_ranges);
    if (n_desc >= (1ull << 30)) return fail(MCBS_ELIMIT, "feature layout: too many columns");
    FeatGeom G{};
    const uint64_t lens[5] = {7u, (uint64_t)b->cfg.maximum_discoverable_credentials_per_action * 4u, (uint64_t)b->cfg.maximum_total_credentials * 2u,
                              (uint64_t)b->cfg.maximum_node_count * b->topo->H()->n_props, b->cfg.maximum_node_count};
    uint64_t V = 0;
    for (int k = 0; k < 5; ++k) { G.len[k] = (uint32_t)lens[k]; G.off[k] = (uint32_t)V; V += lens[k]; }
    uint32_t used = 0;
    std::vector<uint2> elems((size_t)V, make_uint2(0u, 0u));
    std::vector<uint32_t> src_classes((size_t)V, 0u);
    std::vector<FlElem> order;
    bool elems_ok = true;
    uint32_t cur = 0, n_elements = 0;
    for (size_t j = 0; j < n_desc; ++j) {
        const uint32_t d = desc[j], cls = d & (FEAT_MAX_CLASS - 1u), s = (d >> 16) & (FEAT_MAX_SRC - 1u);
        if (s >= V) return fail(MCBS_EINVAL, "feature layout: column %zu reads value %u of %llu per row", j, s, (unsigned long long)V);
        if (d >> 31) {
            if (cls != 0u) return fail(MCBS_EINVAL, "feature layout: column %zu starts an element with class %u", j, cls);
            if (elems[s].y) elems_ok = false;
            elems[s] = make_uint2((uint32_t)j, 1u);
            order.push_back(make_uint4((uint32_t)j, 1u, s, 0u));
            cur = s;
            ++n_elements;
        } else {
            const uint32_t p = j ? desc[j - 1] : 0u;
            if (!j || ((p >> 16) & (FEAT_MAX_SRC - 1u)) != s || (p & (FEAT_MAX_CLASS - 1u)) + 1u != cls)
                return fail(MCBS_EINVAL, "feature layout: column %zu does not continue the element before it (classes 0, 1, 2, ... of one value)", j);
            elems[cur].y += 1u;
            order.back().y += 1u;
        }
        if (cls + 1u > src_classes[s]) src_classes[s] = cls + 1u;
        uint32_t k = 0;
        for (uint32_t q = 1; q < 5u; ++q) k += (uint32_t)(s >= G.off[q]);
        used |= 1u << k;
    }
    const uint64_t A = mcbs_discrete_action_count(b);
    if (n_mask_ranges && A >= (1ull << 31)) return fail(MCBS_ELIMIT, "Discrete action space too large for one launch");
    uint64_t F = n_desc, next_col = 0, top_bit = 0;
    for (size_t r = 0; r < n_mask_ranges; ++r) {
        const uint64_t c0 = mask_ranges[3 * r], n = mask_ranges[3 * r + 1], b0 = mask_ranges[3 * r + 2];
        if (n == 0 || c0 < next_col) return fail(MCBS_EINVAL, "feature layout: mask range %zu is empty or not above the one before it", r);
        if (b0 + n > A) return fail(MCBS_EINVAL, "feature layout: mask range %zu reads bits up to %llu of %llu Discrete actions", r,
                                    (unsigned long long)(b0 + n), (unsigned long long)A);
        G.rc0[r] = (uint32_t)c0; G.rn[r] = (uint32_t)n; G.rb0[r] = (uint32_t)b0;
        next_col = c0 + n;
        F += n;
        if (b0 + n > top_bit) top_bit = b0 + n;
    }
    if (next_col > F) return fail(MCBS_EINVAL, "feature layout: a mask range ends at column %llu of %llu", (unsigned long long)next_col, (unsigned long long)F);
    if (F == 0 || F >= (1ull << 30)) return fail(F ? MCBS_ELIMIT : MCBS_EINVAL, "feature layout: %llu columns", (unsigned long long)F);
    G.F = (uint32_t)F; G.n_desc = (uint32_t)n_desc; G.V = (uint32_t)V; G.n_ranges = (uint32_t)n_mask_ranges;
    G.W = (uint32_t)((top_bit + 31u) / 32u);
    DeviceGuard guard(b->cfg.device);
    if (guard.err != hipSuccess) return fail(MCBS_EHIP, "cannot select device %d: %s", b->cfg.device, hipGetErrorString(guard.err));
    mcbs_feature_layout* l = new (std::nothrow) mcbs_feature_layout();
    if (!l) return fail(MCBS_ENOMEM, "out of memory");
    l->device = b->cfg.device; l->G = G; l->fields_used = used; l->A = A;
    l->n_elements = n_elements; l->src_classes = std::move(src_classes);
    if (n_desc) {
        hipError_t e = hipMalloc(&l->desc_dev, n_desc * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMemcpy(l->desc_dev, desc, n_desc * sizeof(uint32_t), hipMemcpyHostToDevice);
        if (e == hipSuccess && elems_ok) {
            e = hipMalloc(&l->elems_dev, elems.size() * sizeof(uint2));
            if (e == hipSuccess) e = hipMemcpy(l->elems_dev, elems.data(), elems.size() * sizeof(uint2), hipMemcpyHostToDevice);
        }
        if (e == hipSuccess) {
            e = hipMalloc(&l->order_dev, order.size() * sizeof(FlElem));
            if (e == hipSuccess) e = hipMemcpy(l->order_dev, order.data(), order.size() * sizeof(FlElem), hipMemcpyHostToDevice);
        }
        if (e != hipSuccess) {
            if (l->desc_dev) (void)hipFree(l->desc_dev);
            if (l->elems_dev) (void)hipFree(l->elems_dev);
            if (l->order_dev) (void)hipFree(l->order_dev);
            delete l;
            return fail(MCBS_EHIP, "feature layout: descriptor upload failed: %s", hipGetErrorString(e));
        }
    }
    *out = l;
    return MCBS_OK;
}

extern "C" void mcbs_feature_layout_destroy(mcbs_feature_layout* l) {
    if (!l) return;
    DeviceGuard guard(l->device);
    if (l->desc_dev) (void)hipFree(l->desc_dev);
    if (l->elems_dev) (void)hipFree(l->elems_dev);
    if (l->order_dev) (void)hipFree(l->order_dev);
    delete l;
}

extern "C" uint64_t mcbs_feature_layout_width(const mcbs_feature_layout* l) { return l ? l->G.F : 0u; }

extern "C" int mcbs_encode_features(const mcbs_batch* b, const mcbs_feature_layout* l, const mcbs_obs_buffers* obs, const uint32_t* bits,
                                    size_t bits_row_words, void* out, int32_t dtype, size_t out_row_stride, uint64_t n_rows,
                                    uint32_t* out_of_range, void* stream) {
    if (!b || !l || !obs || !out) return fail(MCBS_EINVAL, "null argument");
    MCBS_ON_DEVICE(b);
    if (dtype != MCBS_FEATURES_F32 && dtype != MCBS_FEATURES_BF16 && dtype != MCBS_FEATURES_F16)
        return fail(MCBS_EINVAL, "features dtype must be MCBS_FEATURES_F32, MCBS_FEATURES_BF16 or MCBS_FEATURES_F16");
    const FeatGeom& G = l->G;
    if (l->device != b->cfg.device || l->A != mcbs_discrete_action_count(b) || G.len[1] != b->cfg.maximum_discoverable_credentials_per_action * 4u ||
        G.len[2] != b->cfg.maximum_total_credentials * 2u || G.len[3] != b->cfg.maximum_node_count * b->topo->H()->n_props ||
        G.len[4] != b->cfg.maximum_node_count)
        return fail(MCBS_EINVAL, "mcbs_encode_features: the layout was created for a batch of another device or geometry");
    if (out_row_stride < G.F) return fail(MCBS_EINVAL, "out_row_stride %zu is shorter than the %u feature columns", out_row_stride, G.F);
    FeatSrc src{{obs->scalars, obs->leaked_credentials, obs->credential_cache_matrix, obs->discovered_nodes_properties, obs->nodes_privilegelevel}};
    static const char* const names[5] = {"scalars", "leaked_credentials", "credential_cache_matrix", "discovered_nodes_properties", "nodes_privilegelevel"};
    for (uint32_t k = 0; k < 5u; ++k)
        if (((l->fields_used >> k) & 1u) && !src.f[k]) return fail(MCBS_EINVAL, "mcbs_encode_features: the layout reads obs->%s, which is NULL", names[k]);
    if (G.W) {
        if (!bits) return fail(MCBS_EINVAL, "mcbs_encode_features: the layout has mask columns and bits is NULL");
        if (bits_row_words < G.W) return fail(MCBS_EINVAL, "bits_row_words %zu is shorter than the %u words the layout's mask columns read", bits_row_words, G.W);
    }
    if (n_rows == 0) return MCBS_OK;
    hipStream_t st = (hipStream_t)stream;
    // one wavefront per row, four per workgroup, rows beyond one grid's worth in a loop: about eight workgroups per CU keep the
    // descriptor table's trip into LDS a small share of a workgroup's life
    const dim3 grid = rows_grid(n_rows, 2048u), block(256);
    // the per-element kernel when its LDS fits (element table + four wavefronts' one-hot rows and bit words), else column by column from memory
    const size_t item = dtype == MCBS_FEATURES_F32 ? 4u : 2u, per = 16u / item;
    const size_t lds = (((size_t)G.V + 1u) / 2u + 4u * (((size_t)G.n_desc + per - 1u) / per + ((size_t)G.W + 3u) / 4u)) * 16u;
    const bool rows_kernel = l->elems_dev && lds <= 48u * 1024u;
    const uint32_t one = dtype == MCBS_FEATURES_F32 ? 0x3F800000u : dtype == MCBS_FEATURES_BF16 ? 0x3F80u : 0x3C00u;      // 1.0 as the dtype's pattern
    rows_dispatch<1u, 2u>(item, out, out_row_stride, [&](auto es, auto gw, auto vec) {
        using T = std::conditional_t<decltype(es)::value == 4u, uint32_t, uint16_t>;
        constexpr uint32_t GW = decltype(gw)::value;
        constexpr bool VEC = decltype(vec)::value;
        if (rows_kernel) hipLaunchKernelGGL((encode_features_rows_kernel<T, GW, VEC>), grid, block, lds, st, G, src, l->elems_dev, bits,
                                            bits_row_words, static_cast<T*>(out), out_row_stride, n_rows, (T)one, out_of_range);
        else hipLaunchKernelGGL((encode_features_kernel<T, GW, VEC>), grid, block, 0, st, G, src, l->desc_dev, bits,
                                bits_row_words, static_cast<T*>(out), out_row_stride, n_rows, (T)one, out_of_range);
    });
    return launch_ok("encode features");
}

// ------------------------------------------------------------------ packed observations
struct mcbs_obs_packing {
    int32_t device = 0;
    ObsPackGeom P{};
    uint32_t* desc_dev = nullptr;
    uint32_t* word_first_dev = nullptr;     // [W + 1] first value index of each word (| FUSED_WORD_PROPS), behind the descriptors in one allocation
    std::vector<uint32_t> valid;    // per source value: its valid codes
};

// ints per row of the five int32 observation fields of a batch
static void obs_field_lens(const mcbs_batch* b, uint64_t (&lens)[5]) {
    lens[0] = 7u;
    lens[1] = (uint64_t)b->cfg.maximum_discoverable_credentials_per_action * 4u;
    lens[2] = (uint64_t)b->cfg.maximum_total_credentials * 2u;
    lens[3] = (uint64_t)b->cfg.maximum_node_count * b->topo->H()->n_props;
    lens[4] = b->cfg.maximum_node_count;
}
static bool obs_packing_fits(const mcbs_batch* b, const mcbs_obs_packing* p) {
    uint64_t lens[5];
    obs_field_lens(b, lens);
    bool same = p->device == b->cfg.device;
    for (int k = 0; k < 5; ++k) same = same && p->P.len[k] == lens[k];
    return same;
}

extern "C" int mcbs_obs_packing_create(const mcbs_batch* b, const uint32_t* valid_codes, size_t n_values, mcbs_obs_packing** out) {
    if (!b || !valid_codes || !out) return fail(MCBS_EINVAL, "null argument");
    ObsPackGeom P{};
    uint64_t lens[5], V = 0;
    obs_field_lens(b, lens);
    for (int k = 0; k < 5; ++k) { P.len[k] = (uint32_t)lens[k]; P.off[k] = (uint32_t)V; V += lens[k]; }
    if (n_values != V) return fail(MCBS_EINVAL, "observation packing: %zu valid-code counts for the %llu values of a row", n_values, (unsigned long long)V);
    std::vector<uint32_t> desc(n_values), word_first(1, 0u);       // word_first[w]: the first value of word w; the last entry: V
    uint64_t word = 0;
    uint32_t shift = 0;                                    // the next free bit is bit `shift` of word `word`
    for (size_t s = 0; s < n_values; ++s) {
        const uint32_t n = valid_codes[s];
        if (n == 0u || n > OBS_PACK_MAX_CODES) return fail(MCBS_ELIMIT, "observation packing: value %zu has %u valid codes (1 to %u)", s, n, OBS_PACK_MAX_CODES);
        uint32_t width = 0;
        while ((n >> width) != 0u) ++width;                // bit_length(n)
        if (shift + width > 32u) { ++word; shift = 0; word_first.push_back((uint32_t)s); }    // a field never straddles a word
        if (word >= OBS_PACK_MAX_WORDS) return fail(MCBS_ELIMIT, "observation packing: a row needs more than %u words", OBS_PACK_MAX_WORDS);
        desc[s] = (n - 1u) | (((uint32_t)word * 32u + shift) << 16);
        shift += width;
    }
    P.V = (uint32_t)V;
    P.W = (uint32_t)word + (shift ? 1u : 0u);
    word_first.resize(P.W);                                // (V == 0: no word)
    word_first.push_back(P.V);
    // the packed wrapper step (mcbs_wrapper_fused.hip) builds a word of two-code property values as a bit-spread: flag those words
    for (uint32_t w = 0; w < P.W; ++w) {
        const uint32_t first = word_first[w], last = word_first[w + 1u] & ~FUSED_WORD_PROPS;
        bool props = first >= P.off[3] && last <= P.off[3] + P.len[3];
        for (uint32_t s = first; props && s < last; ++s) props = valid_codes[s] == 2u;
        if (props) word_first[w] |= FUSED_WORD_PROPS;
    }
    desc.insert(desc.end(), word_first.begin(), word_first.end());       // one upload: descriptors [V] | word_first [W + 1]
    DeviceGuard guard(b->cfg.device);
    if (guard.err != hipSuccess) return fail(MCBS_EHIP, "cannot select device %d: %s", b->cfg.device, hipGetErrorString(guard.err));
    mcbs_obs_packing* p = new (std::nothrow) mcbs_obs_packing();
    if (!p) return fail(MCBS_ENOMEM, "out of memory");
    p->device = b->cfg.device; p->P = P; p->valid.assign(valid_codes, valid_codes + n_values);
    hipError_t e = hipMalloc(&p->desc_dev, desc.size() * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemcpy(p->desc_dev, desc.data(), desc.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    p->word_first_dev = p->desc_dev ? p->desc_dev + n_values : nullptr;
    if (e != hipSuccess) {
        if (p->desc_dev) (void)hipFree(p->desc_dev);
        delete p;
        return fail(MCBS_EHIP, "observation packing: descriptor upload failed: %s", hipGetErrorString(e));
    }
    *out = p;
    return MCBS_OK;
}

extern "C" void mcbs_obs_packing_destroy(mcbs_obs_packing* p) {
    if (!p) return;
    DeviceGuard guard(p->device);
    if (p->desc_dev) (void)hipFree(p->desc_dev);
    delete p;
}

extern "C" uint64_t mcbs_obs_packing_words(const mcbs_obs_packing* p) { return p ? p->P.W : 0u; }

extern "C" int mcbs_pack_observation(const mcbs_batch* b, const mcbs_obs_packing* p, const mcbs_obs_buffers* obs, uint32_t* out,
                                     size_t out_row_words, uint64_t n_rows, uint32_t* out_of_range, void* stream) {
    if (!b || !p || !obs || !out) return fail(MCBS_EINVAL, "null argument");
    MCBS_ON_DEVICE(b);
    if (!obs_packing_fits(b, p)) return fail(MCBS_EINVAL, "mcbs_pack_observation: the packing was created for a batch of another device or geometry");
    FeatSrc src{{obs->scalars, obs->leaked_credentials, obs->credential_cache_matrix, obs->discovered_nodes_properties, obs->nodes_privilegelevel}};
    for (uint32_t k = 0; k < 5u; ++k)
        if (!src.f[k]) return fail(MCBS_EINVAL, "mcbs_pack_observation: all five int32 fields are packed, field %u is NULL", k);
    if (out_row_words < p->P.W) return fail(MCBS_EINVAL, "out_row_words %zu is shorter than the %u words of a packed row", out_row_words, p->P.W);
    if (n_rows == 0) return MCBS_OK;
    hipLaunchKernelGGL(pack_observation_kernel, rows_grid(n_rows, 2048u), dim3(256), 4u * p->P.W * sizeof(uint32_t), (hipStream_t)stream, p->P, src,
                       p->desc_dev, out, out_row_words, n_rows, out_of_range);
    return launch_ok("pack observation");
}

extern "C" int mcbs_unpack_observation(const mcbs_batch* b, const mcbs_obs_packing* p, const uint32_t* packed, size_t row_words,
                                       const int64_t* index, uint64_t n_source_rows, uint64_t n_rows, const mcbs_obs_buffers* out, void* stream) {
    if (!b || !p || !packed || !out) return fail(MCBS_EINVAL, "null argument");
    MCBS_ON_DEVICE(b);
    if (!obs_packing_fits(b, p)) return fail(MCBS_EINVAL, "mcbs_unpack_observation: the packing was created for a batch of another device or geometry");
    if (row_words < p->P.W) return fail(MCBS_EINVAL, "row_words %zu is shorter than the %u words of a packed row", row_words, p->P.W);
    if (!index && n_rows > n_source_rows) return fail(MCBS_EINVAL, "mcbs_unpack_observation: %llu rows asked of %llu stored ones and no index",
                                                      (unsigned long long)n_rows, (unsigned long long)n_source_rows);
    if (n_rows == 0) return MCBS_OK;
    ObsDst dst{{out->scalars, out->leaked_credentials, out->credential_cache_matrix, out->discovered_nodes_properties, out->nodes_privilegelevel}};
    hipLaunchKernelGGL(unpack_observation_kernel, rows_grid(n_rows, 2048u), dim3(256), 0, (hipStream_t)stream, p->P, p->desc_dev, packed, row_words,
                       index, n_source_rows, dst, n_rows);
    return launch_ok("unpack observation");
}

// The one-launch wrapper step with the packed store side (mcbs_wrapper_fused.hip wrapper_fused_packed_kernel): the argument block of
// the int32 step with no observation field (fused_wrapper_args), and the packed rows' own.  Every check before the launch: a refused
// call launches nothing and changes no state.
extern "C" int mcbs_attacker_wrapper_step_packed(mcbs_batch* b, const int64_t* multidiscrete, const int64_t* discrete, int32_t* decoded,
                                                 const mcbs_info_buffers* info, const mcbs_obs_packing* p, uint32_t* packed, uint32_t* packed_terminal,
                                                 const uint32_t* packed_fresh, size_t row_words, const mcbs_wrapper_buffers* w, float modifier,
                                                 int32_t max_timesteps, int32_t auto_reset, void* stream) {
    const char* who = "mcbs_attacker_wrapper_step_packed";
    if (!b || !w || !decoded || !p || !packed) return fail(MCBS_EINVAL, "null argument");
    MCBS_ON_DEVICE(b);
    StepIO io;
    int rc = attacker_turn_io(b, multidiscrete, discrete, decoded, info, w, modifier, max_timesteps, auto_reset, nullptr, nullptr, &io);
    if (rc) return rc;
    if (!b->variant.fused_wrapper)
        return fail(MCBS_EINVAL, "%s: the wrapper step of this batch is not one launch (packed batch, at most 16 nodes and cached credentials, not "
                                 "the random-events defender); there is no multi-launch form of the packed step", who);
    if (!obs_packing_fits(b, p)) return fail(MCBS_EINVAL, "%s: the packing was created for a batch of another device or geometry", who);
    const uint32_t W = p->P.W, V = p->P.V;
    if (row_words < W) return fail(MCBS_EINVAL, "row_words %zu is shorter than the %u words of a packed row", row_words, W);
    if (W > FUSED_PACKED_MAX_WORDS || W + 1u + V > FUSED_PACKED_TABLE_DWORDS)
        return fail(MCBS_EINVAL, "%s: a packed row of %u words and %u values is beyond the LDS room the step keeps for the fresh row (%u words) and "
                                 "its tables (%u entries)", who, W, V, FUSED_PACKED_MAX_WORDS, FUSED_PACKED_TABLE_DWORDS);
    if (auto_reset && (!packed_terminal || !packed_fresh))
        return fail(MCBS_EINVAL, "%s: auto_reset needs packed_terminal (the rows of the envs that end) and packed_fresh (the row of a reset env)", who);
    if (!auto_reset) packed_terminal = nullptr, packed_fresh = nullptr;                 // (neither is touched)
    // the three arrays this entry point adds may share no byte with each other, with an input or with an array of `w` / `info`, which the
    // same launch writes (those are listed as not written: unlike the training turn, this call does not refuse two of them against each other)
    const uint64_t E = b->S.E;
    Extents ext;
    ext.rows("packed", packed, E, row_words, W, 4u, true); ext.rows("packed_terminal", packed_terminal, E, row_words, W, 4u, true);
    ext.bytes("decoded", decoded, E * 20u, true); ext.bytes("packed_fresh", packed_fresh, (uint64_t)W * 4u, false);
    ext.bytes("multidiscrete", multidiscrete, E * 80u, false); ext.bytes("discrete", discrete, E * 8u, false);
    add_arrays(ext, "w->", w, kWrapperArrays, E, 0u, 0u, false);
    add_arrays(ext, "info->", info, kInfoArrays, E, 0u, 0u, false);
    if ((rc = disjoint(who, ext))) return rc;
    const mcbs_obs_buffers none{};
    FusedArgs A;
    if (!fused_wrapper_args(b, multidiscrete, discrete, decoded, &none, w, modifier, max_timesteps, auto_reset, nullptr, nullptr, &A))
        return fail(MCBS_EINVAL, "%s: the wrapper step of this batch is not one launch", who);
    FusedPackedArgs PA{};
    PA.packed = packed; PA.term = packed_terminal; PA.fresh = packed_fresh; PA.desc = p->desc_dev; PA.word_first = p->word_first_dev;
    PA.row_words = row_words; PA.W = W; PA.V = V;
    PA.off1 = p->P.off[1]; PA.off2 = p->P.off[2]; PA.off3 = p->P.off[3]; PA.off4 = p->P.off[4];
    b->all_fresh = false;
    const dim3 grid((b->S.E + 63u) / 64u), block(FUSED_THREADS);
    pick<MCBS_DEFENDER_SCAN_AND_REIMAGE, MCBS_DEFENDER_EXTERNAL, MCBS_DEFENDER_NONE>((int)b->cfg.defender_kind, [&](auto def) {
        hipLaunchKernelGGL((wrapper_fused_packed_kernel<decltype(def)::value>), grid, block, 0, (hipStream_t)stream, b->S, b->T, b->C_dev, io, A, PA);
    });
    return turn_launched(b, "wrapper step (one launch, packed rows)");
}

extern "C" int mcbs_encode_features_packed(const mcbs_batch* b, const mcbs_feature_layout* l, const mcbs_obs_packing* p, const uint32_t* packed,
                                           size_t packed_row_words, const uint32_t* bits, size_t bits_row_words, const int64_t* index,
                                           uint64_t n_source_rows, void* out, int32_t dtype, size_t out_row_stride, uint64_t n_rows,
                                           uint32_t* out_of_range, void* stream) {
    if (!b || !l || !p || !packed || !out) return fail(MCBS_EINVAL, "null argument");
    MCBS_ON_DEVICE(b);
    if (dtype != MCBS_FEATURES_F32 && dtype != MCBS_FEATURES_BF16 && dtype != MCBS_FEATURES_F16)
        return fail(MCBS_EINVAL, "features dtype must be MCBS_FEATURES_F32, MCBS_FEATURES_BF16 or MCBS_FEATURES_F16");
    const FeatGeom& G = l->G;
    bool same = obs_packing_fits(b, p) && l->device == b->cfg.device && l->A == mcbs_discrete_action_count(b);
    for (int k = 0; k < 5; ++k) same = same && G.len[k] == p->P.len[k];
    if (!same) return fail(MCBS_EINVAL, "mcbs_encode_features_packed: the layout or the packing was created for a batch of another device or geometry");
    for (size_t s = 0; s < p->valid.size(); ++s)
        if (l->src_classes[s] > p->valid[s])
            return fail(MCBS_EINVAL, "mcbs_encode_features_packed: the layout gives value %zu %u classes, the packing %u valid codes", s,
                        l->src_classes[s], p->valid[s]);
    if (out_row_stride < G.F) return fail(MCBS_EINVAL, "out_row_stride %zu is shorter than the %u feature columns", out_row_stride, G.F);
    if (packed_row_words < p->P.W) return fail(MCBS_EINVAL, "packed_row_words %zu is shorter than the %u words of a packed row", packed_row_words, p->P.W);
    if (G.W) {
        if (!bits) return fail(MCBS_EINVAL, "mcbs_encode_features_packed: the layout has mask columns and bits is NULL");
        if (bits_row_words < G.W) return fail(MCBS_EINVAL, "bits_row_words %zu is shorter than the %u words the layout's mask columns read", bits_row_words, G.W);
    }
    if (!index && n_rows > n_source_rows) return fail(MCBS_EINVAL, "mcbs_encode_features_packed: %llu rows asked of %llu stored ones and no index",
                                                      (unsigned long long)n_rows, (unsigned long long)n_source_rows);
    if (n_rows == 0) return MCBS_OK;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid = rows_grid(n_rows, 2048u), block(256);        // (as mcbs_encode_features)
    // the per-element kernel when its LDS fits (as mcbs_encode_features chooses), else column by column: on four wavefronts' decoded rows
    // in LDS when those fit, else decoding where a column asks
    const size_t item = dtype == MCBS_FEATURES_F32 ? 4u : 2u, per = 16u / item;
    const size_t lds_rows = (((size_t)G.V + 1u) / 2u + 4u * (((size_t)G.n_desc + per - 1u) / per + ((size_t)G.W + 3u) / 4u)) * 16u;
    const bool rows_kernel = l->elems_dev && lds_rows <= 48u * 1024u;
    const size_t lds = 4u * (size_t)G.V * sizeof(uint32_t);
    const bool staged = lds <= 48u * 1024u;
    const uint32_t one = dtype == MCBS_FEATURES_F32 ? 0x3F800000u : dtype == MCBS_FEATURES_BF16 ? 0x3F80u : 0x3C00u;      // 1.0 as the dtype's pattern
    rows_dispatch<1u, 2u>(item, out, out_row_stride, [&](auto es, auto gw, auto vec) {
        using T = std::conditional_t<decltype(es)::value == 4u, uint32_t, uint16_t>;
        constexpr uint32_t GW = decltype(gw)::value;
        constexpr bool VEC = decltype(vec)::value;
        if (rows_kernel) hipLaunchKernelGGL((encode_features_packed_rows_kernel<T, GW, VEC>), grid, block, lds_rows, st, G, l->elems_dev, l->n_elements,
                                            p->desc_dev, packed, packed_row_words, bits, bits_row_words, index, n_source_rows, static_cast<T*>(out),
                                            out_row_stride, n_rows, (T)one, out_of_range);
        else if (staged) hipLaunchKernelGGL((encode_features_packed_kernel<T, GW, VEC, true>), grid, block, lds, st, G, l->desc_dev, l->n_elements, p->desc_dev,
                                       packed, packed_row_words, bits, bits_row_words, index, n_source_rows, static_cast<T*>(out), out_row_stride,
                                       n_rows, (T)one, out_of_range);
        else hipLaunchKernelGGL((encode_features_packed_kernel<T, GW, VEC, false>), grid, block, 0, st, G, l->desc_dev, l->n_elements, p->desc_dev,
                                packed, packed_row_words, bits, bits_row_words, index, n_source_rows, static_cast<T*>(out), out_row_stride,
                                n_rows, (T)one, out_of_range);
    });
    return launch_ok("encode features from packed observations");
}

// ------------------------------------------------------------------ first layer from the observation
static const char* const kObsFields[5] = {"scalars", "leaked_credentials", "credential_cache_matrix", "discovered_nodes_properties", "nodes_privilegelevel"};
// The checks on (batch, layout, source) the three calls share; fills S and appends the source's extents.  obs: the dense form; else
// packing + packed (+ index).
static int fl_source(const char* who, const mcbs_batch* b, const mcbs_feature_layout* l, const mcbs_obs_buffers* obs, const mcbs_obs_packing* p,
                     const uint32_t* packed, size_t packed_row_words, const int64_t* index, uint64_t n_source_rows, uint64_t n_rows, FlSrc& S,
                     Extents& ext) {
    const FeatGeom& G = l->G;
    if (G.n_ranges || G.W) return fail(MCBS_EINVAL, "%s: the layout has mask columns; include_masks is out of scope of the first-layer calls", who);
    uint64_t lens[5];
    obs_field_lens(b, lens);
    bool same = l->device == b->cfg.device && l->A == mcbs_discrete_action_count(b);
    for (int k = 0; k < 5; ++k) same = same && G.len[k] == lens[k];
    if (!same) return fail(MCBS_EINVAL, "%s: the layout was created for a batch of another device or geometry", who);
    S = FlSrc{};
    if (obs) {
        S.dense = FeatSrc{{obs->scalars, obs->leaked_credentials, obs->credential_cache_matrix, obs->discovered_nodes_properties, obs->nodes_privilegelevel}};
        for (uint32_t k = 0; k < 5u; ++k) {
            if (!((l->fields_used >> k) & 1u)) { S.dense.f[k] = nullptr; continue; }
            if (!S.dense.f[k]) return fail(MCBS_EINVAL, "%s: the layout reads obs->%s, which is NULL", who, kObsFields[k]);
            ext.bytes(kObsFields[k], S.dense.f[k], n_rows * G.len[k] * 4u, false);
        }
        return MCBS_OK;
    }
    if (!p || !packed) return fail(MCBS_EINVAL, "%s: packing or packed is NULL", who);
    if (!obs_packing_fits(b, p)) return fail(MCBS_EINVAL, "%s: the packing was created for a batch of another device or geometry", who);
    for (size_t s = 0; s < p->valid.size(); ++s)
        if (l->src_classes[s] > p->valid[s])
            return fail(MCBS_EINVAL, "%s: the layout gives value %zu %u classes, the packing %u valid codes", who, s, l->src_classes[s], p->valid[s]);
    if (packed_row_words < p->P.W) return fail(MCBS_EINVAL, "%s: packed_row_words %zu is shorter than the %u words of a packed row", who, packed_row_words, p->P.W);
    if (!index && n_rows > n_source_rows)
        return fail(MCBS_EINVAL, "%s: %llu rows asked of %llu stored ones and no index", who, (unsigned long long)n_rows, (unsigned long long)n_source_rows);
    S.pdesc = p->desc_dev; S.packed = packed; S.packed_row_words = packed_row_words; S.index = index; S.n_source_rows = n_source_rows;
    ext.rows("packed", packed, n_source_rows, packed_row_words, p->P.W, 4u, false);
    ext.bytes("index", index, n_rows * 8u, false);
    return MCBS_OK;
}

static int first_layer_forward(const char* who, const mcbs_batch* b, const mcbs_feature_layout* l, const mcbs_obs_buffers* obs, const mcbs_obs_packing* p,
                               const uint32_t* packed, size_t packed_row_words, const int64_t* index, uint64_t n_source_rows, uint64_t n_rows,
                               const void* weight_t, size_t weight_row_stride, const void* bias, int32_t weight_dtype, uint32_t H, void* out,
                               int32_t out_dtype, size_t out_row_stride, uint32_t* out_of_range, void* stream) {
    if (H < 1u || H > MCBS_LINEAR_MAX_H) return fail(MCBS_EINVAL, "%s: H %u: from 1 to %u", who, H, (uint32_t)MCBS_LINEAR_MAX_H);
    if ((weight_dtype != MCBS_FEATURES_F32 && weight_dtype != MCBS_FEATURES_BF16) || (out_dtype != MCBS_FEATURES_F32 && out_dtype != MCBS_FEATURES_BF16))
        return fail(MCBS_EINVAL, "%s: weight_dtype and out_dtype must be MCBS_FEATURES_F32 or MCBS_FEATURES_BF16", who);
    if (!weight_t || !out) return fail(MCBS_EINVAL, "%s: weight_t and out must not be NULL", who);
    if (weight_row_stride < H) return fail(MCBS_EINVAL, "%s: weight_row_stride %zu is shorter than H = %u", who, weight_row_stride, H);
    if (out_row_stride < H) return fail(MCBS_EINVAL, "%s: out_row_stride %zu is shorter than H = %u", who, out_row_stride, H);
    FlSrc S;
    Extents ext;
    const size_t wes = weight_dtype == MCBS_FEATURES_F32 ? 4u : 2u, oes = out_dtype == MCBS_FEATURES_F32 ? 4u : 2u;
    ext.rows("out", out, n_rows, out_row_stride, H, oes, true);
    ext.rows("weight_t", weight_t, l->G.F, weight_row_stride, H, wes, false);
    ext.bytes("bias", bias, H * wes, false);
    ext.bytes("out_of_range", out_of_range, 4u, false);
    int rc;
    if ((rc = fl_source(who, b, l, obs, p, packed, packed_row_words, index, n_source_rows, n_rows, S, ext))) return rc;
    if ((rc = disjoint(who, ext))) return rc;
    if (n_rows == 0) return MCBS_OK;
    const uint64_t groups = (n_rows + FL_ROWS - 1u) / FL_ROWS;
    if (groups > 0x7FFFFFFFull) return fail(MCBS_EINVAL, "%s: too many rows", who);
    const dim3 grid((uint32_t)groups, (H + 63u) / 64u), block(256);
    hipStream_t st = (hipStream_t)stream;
    pick<2, 4>((int)wes, [&](auto we) {
        using WT = std::conditional_t<decltype(we)::value == 4, float, uint16_t>;
        pick<2, 4>((int)oes, [&](auto oe) {
            using OT = std::conditional_t<decltype(oe)::value == 4, float, uint16_t>;
            pick<0, 1>(obs ? 0 : 1, [&](auto pk) {
                hipLaunchKernelGGL((first_layer_kernel<WT, OT, decltype(pk)::value != 0>), grid, block, 0, st, l->G, S, l->order_dev, l->n_elements,
                                   static_cast<const WT*>(weight_t), weight_row_stride, static_cast<const WT*>(bias), H, static_cast<OT*>(out),
                                   out_row_stride, n_rows, out_of_range);
            });
        });
    });
    return launch_ok("first layer");
}

extern "C" int mcbs_first_layer(const mcbs_batch* b, const mcbs_feature_layout* l, const mcbs_obs_buffers* obs, uint64_t n_rows, const void* weight_t,
                                size_t weight_row_stride, const void* bias, int32_t weight_dtype, uint32_t H, void* out, int32_t out_dtype,
                                size_t out_row_stride, uint32_t* out_of_range, void* stream) {
    if (!b || !l || !obs) return fail(MCBS_EINVAL, "mcbs_first_layer: null argument");
    MCBS_ON_DEVICE(b);
    return first_layer_forward("mcbs_first_layer", b, l, obs, nullptr, nullptr, 0u, nullptr, 0u, n_rows, weight_t, weight_row_stride, bias, weight_dtype, H,
                               out, out_dtype, out_row_stride, out_of_range, stream);
}

extern "C" int mcbs_first_layer_packed(const mcbs_batch* b, const mcbs_feature_layout* l, const mcbs_obs_packing* p, const uint32_t* packed,
                                       size_t packed_row_words, const int64_t* index, uint64_t n_source_rows, uint64_t n_rows, const void* weight_t,
                                       size_t weight_row_stride, const void* bias, int32_t weight_dtype, uint32_t H, void* out, int32_t out_dtype,
                                       size_t out_row_stride, uint32_t* out_of_range, void* stream) {
    if (!b || !l || !p || !packed) return fail(MCBS_EINVAL, "mcbs_first_layer_packed: null argument");
    MCBS_ON_DEVICE(b);
    return first_layer_forward("mcbs_first_layer_packed", b, l, nullptr, p, packed, packed_row_words, index, n_source_rows, n_rows, weight_t,
                               weight_row_stride, bias, weight_dtype, H, out, out_dtype, out_row_stride, out_of_range, stream);
}

extern "C" size_t mcbs_first_layer_grad_workspace(const mcbs_batch* b, const mcbs_feature_layout* l, uint64_t n_rows, uint32_t H) {
    if (!b || !l || l->G.n_ranges || l->G.W || H < 1u || H > MCBS_LINEAR_MAX_H) return 0;
    const uint64_t n_blocks = (n_rows + MCBS_FIRST_LAYER_GRAD_ROW_BLOCK - 1u) / MCBS_FIRST_LAYER_GRAD_ROW_BLOCK;
    return (size_t)n_blocks * ((size_t)l->G.F + 1u) * H * sizeof(float);
}

extern "C" int mcbs_first_layer_grad(const mcbs_batch* b, const mcbs_feature_layout* l, const mcbs_obs_buffers* obs, const mcbs_obs_packing* p,
                                     const uint32_t* packed, size_t packed_row_words, const int64_t* index, uint64_t n_source_rows, uint64_t n_rows,
                                     const float* grad_out, size_t grad_out_row_stride, uint32_t H, float* grad_weight_t, size_t grad_weight_row_stride,
                                     float* grad_bias, void* workspace, size_t workspace_bytes, void* stream) {
    static const char* who = "mcbs_first_layer_grad";
    static_assert(FLG_ROW_BLOCK == MCBS_FIRST_LAYER_GRAD_ROW_BLOCK, "the kernel's row block is the header's");
    if (!b || !l) return fail(MCBS_EINVAL, "%s: null argument", who);
    MCBS_ON_DEVICE(b);
    if ((obs != nullptr) == (p != nullptr || packed != nullptr))
        return fail(MCBS_EINVAL, "%s: give either obs (the dense fields) or packing and packed, not both and not neither", who);
    if (H < 1u || H > MCBS_LINEAR_MAX_H) return fail(MCBS_EINVAL, "%s: H %u: from 1 to %u", who, H, (uint32_t)MCBS_LINEAR_MAX_H);
    if (!grad_weight_t && !grad_bias) return fail(MCBS_EINVAL, "%s: grad_weight_t and grad_bias are both NULL", who);
    if (grad_weight_t && grad_weight_row_stride < H) return fail(MCBS_EINVAL, "%s: grad_weight_row_stride %zu is shorter than H = %u", who, grad_weight_row_stride, H);
    if (n_rows) {
        if (!grad_out) return fail(MCBS_EINVAL, "%s: grad_out must not be NULL", who);
        if (grad_out_row_stride < H) return fail(MCBS_EINVAL, "%s: grad_out_row_stride %zu is shorter than H = %u", who, grad_out_row_stride, H);
    }
    FlSrc S;
    Extents ext;
    const uint32_t F = l->G.F;
    const size_t need = mcbs_first_layer_grad_workspace(b, l, n_rows, H);
    ext.rows("grad_weight_t", grad_weight_t, F, grad_weight_row_stride, H, 4u, true);
    ext.bytes("grad_bias", grad_bias, H * 4u, true);
    ext.bytes("workspace", workspace, need, true);
    ext.rows("grad_out", grad_out, n_rows, grad_out_row_stride, H, 4u, false);
    int rc;
    if ((rc = fl_source(who, b, l, obs, p, packed, packed_row_words, index, n_source_rows, n_rows, S, ext))) return rc;
    if (need && (!workspace || workspace_bytes < need))
        return fail(MCBS_EINVAL, "%s: the workspace must hold %zu bytes (mcbs_first_layer_grad_workspace), got %zu at %p", who, need, workspace_bytes, workspace);
    if ((rc = disjoint(who, ext))) return rc;
    const uint64_t n_blocks = (n_rows + FLG_ROW_BLOCK - 1u) / FLG_ROW_BLOCK;
    const uint32_t n_slabs = grad_weight_t ? (l->n_elements + FLG_WAVES * FLG_EPW - 1u) / (FLG_WAVES * FLG_EPW) : 1u;
    if (n_blocks * (n_slabs ? n_slabs : 1u) > 0x7FFFFFFFull) return fail(MCBS_EINVAL, "%s: too many rows", who);
    hipStream_t st = (hipStream_t)stream;
    float* partials = static_cast<float*>(workspace);
    if (n_rows) {
        const dim3 grid((uint32_t)n_blocks * (n_slabs ? n_slabs : 1u), (H + 63u) / 64u), block(256);
        pick<0, 1>(obs ? 0 : 1, [&](auto pk) {
            hipLaunchKernelGGL((first_layer_grad_kernel<decltype(pk)::value != 0>), grid, block, 0, st, l->G, S, l->order_dev, l->n_elements,
                               n_slabs ? n_slabs : 1u, grad_out, grad_out_row_stride, H, partials, n_rows, grad_weight_t != nullptr, grad_bias != nullptr);
        });
    }
    const uint64_t cells = ((uint64_t)F + 1u) * H, blocks = (cells + 255u) / 256u;
    hipLaunchKernelGGL(first_layer_grad_reduce_kernel, dim3(blocks < 65536u ? (uint32_t)blocks : 65536u), dim3(256), 0, st, partials, (uint32_t)n_blocks, F, H,
                       grad_weight_t, grad_weight_row_stride, grad_bias);
    return launch_ok("first layer gradient");
}

// ------------------------------------------------------------------ learned defender
// The observation written by the turn kernel's own workgroups (variant.fused_defender_obs): output arrays on 16-byte boundaries (the 128
// envs of a workgroup are one contiguous region of each array, stored as 16-byte vectors)
static DefObs fused_defender_obs(const mcbs_batch* b, const mcbs_defender_obs* o) {
    DefObs d{};
    if (!o) return d;
    d.infected = o->infected_nodes; d.fw_in = o->incoming_firewall_status; d.fw_out = o->outgoing_firewall_status; d.services = o->services_status;
    d.n_services = b->C.n_services;
    const uint32_t N = b->S.N ? b->S.N : 1u;
    d.dN = fast_div_host(N); d.d6N = fast_div_host(6u * N); d.dS = fast_div_host(d.n_services ? d.n_services : 1u);
    auto al = [](const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; };
    const bool aligned = al(d.infected) && al(d.fw_in) && al(d.fw_out) && al(d.services);
    d.fused = (b->variant.fused_defender_obs && aligned) ? 1u : 0u;
    return d;
}

static int launch_defender_obs(mcbs_batch* b, const mcbs_defender_obs* o, hipStream_t st) {
    const uint32_t total = b->S.E * b->S.N;
    hipLaunchKernelGGL(defender_obs_kernel, dim3((total + 255) / 256), dim3(256), 0, st, b->S, b->T, o->infected_nodes,
                       o->incoming_firewall_status, o->outgoing_firewall_status, o->services_status, b->C.n_services);
    return launch_ok("defender observation");
}

static int learned_defender_ok(const mcbs_batch* b) {
    if (b->cfg.defender_kind != MCBS_DEFENDER_EXTERNAL) return fail(MCBS_ESTATE, "batch was not created with MCBS_DEFENDER_EXTERNAL");
    return MCBS_OK;
}

// One turn of the learned defender: 128 envs per workgroup, launch(WT, grid, block, observation arguments) for the batch's words per set;
// then the observation as a launch of its own where the turn kernel could not write it.  obs == nullptr: no dense observation is asked for —
// also the call of a kernel that writes an observation of its own (the packed rows) and ignores the DefObs it is handed
template <class Launch>
static int launch_defender_turn(mcbs_batch* b, const mcbs_defender_obs* obs, hipStream_t st, const char* what, Launch&& launch) {
    b->all_fresh = false;
    const DefObs dob = fused_defender_obs(b, obs);
    pick<1, 2, 4>((int)b->S.WT, [&](auto wt) { launch(wt, dim3((b->S.E + 127) / 128), dim3(128), dob); });
    const int rc = launch_ok(what);
    if (rc || !obs || dob.fused) return rc;
    return launch_defender_obs(b, obs, st);
}

extern "C" int mcbs_defender_step(mcbs_batch* b, const int64_t* actions, uint8_t* valid, double* availability, uint8_t* evicted,
                                  const mcbs_defender_obs* obs, void* stream) {
    if (!b || !actions) return fail(MCBS_EINVAL, "null argument");
    MCBS_ON_DEVICE(b);
    if (const int rc = learned_defender_ok(b)) return rc;
    return launch_defender_turn(b, obs, (hipStream_t)stream, "defender step", [&](auto wt, dim3 grid, dim3 block, const DefObs& dob) {
        hipLaunchKernelGGL((defender_kernel<decltype(wt)::value>), grid, block, 0, (hipStream_t)stream, b->S, b->T, b->C_dev, actions, valid, availability, evicted, dob);
    });
}

extern "C" int mcbs_defender_wrapper_step(mcbs_batch* b, const int64_t* actions, const mcbs_defender_obs* obs, const mcbs_defender_wrapper_buffers* w,
                                          const mcbs_defender_wrapper_cfg* cfg, void* stream) {
    if (!b || !actions || !w || !cfg) return fail(MCBS_EINVAL, "null argument");
    MCBS_ON_DEVICE(b);
    if (const int rc = learned_defender_ok(b)) return rc;
    if (!arrays_set(w, 0)) return fail(MCBS_EINVAL, "mcbs_defender_wrapper_buffers: every array is required");
    return launch_defender_turn(b, obs, (hipStream_t)stream, "defender turn + reward shaping", [&](auto wt, dim3 grid, dim3 block, const DefObs& dob) {
        hipLaunchKernelGGL((defender_turn_post_kernel<decltype(wt)::value>), grid, block, 0, (hipStream_t)stream, b->S, b->T, b->C_dev, actions, *w, *cfg, dob);
    });
}

extern "C" int mcbs_defender_observe(mcbs_batch* b, const mcbs_defender_obs* obs, void* stream) {
    if (!b || !obs) return fail(MCBS_EINVAL, "null argument");
    MCBS_ON_DEVICE(b);
    if (const int rc = learned_defender_ok(b)) return rc;
    return launch_defender_obs(b, obs, (hipStream_t)stream);
}

// ------------------------------------------------------------------ packed defender observations (mcbs_defender_obs_packing.hip)
// the checks every call on packed defender rows shares: a learned defender's batch, rows of at least W_def words
static int defender_packing_ok(const mcbs_batch* b, const char* who, size_t row_words) {
    if (b->cfg.defender_kind != MCBS_DEFENDER_EXTERNAL) return fail(MCBS_EINVAL, "%s: batch was not created with MCBS_DEFENDER_EXTERNAL", who);
    if (row_words < b->def_pack.W) return fail(MCBS_EINVAL, "%s: row_words %zu is shorter than the %u words of a packed defender row", who, row_words, b->def_pack.W);
    return MCBS_OK;
}
static bool defender_obs_complete(const mcbs_defender_obs* o) {
    return o->infected_nodes && o->incoming_firewall_status && o->outgoing_firewall_status && o->services_status;
}
// the four fields in the packed row's COLUMN order, as the kernels read (DefDense) or write (DefDenseOut) them
template <class D = DefDense>
static D def_dense(const mcbs_defender_obs* o) { return D{{o->incoming_firewall_status, o->infected_nodes, o->outgoing_firewall_status, o->services_status}}; }

extern "C" uint32_t mcbs_defender_obs_words(const mcbs_batch* b) {
    return (b && b->cfg.defender_kind == MCBS_DEFENDER_EXTERNAL) ? b->def_pack.W : 0u;
}

// defender_obs_packed_kernel takes a thread per (env, word) of one launch: checked before anything is launched
static int defender_live_rows_ok(const mcbs_batch* b) {
    const uint64_t total = (uint64_t)b->S.E * b->def_pack.W;
    if (total >= (1ull << 32)) return fail(MCBS_ELIMIT, "packed defender observation: %llu words in one launch", (unsigned long long)total);
    return MCBS_OK;
}
static int launch_defender_obs_packed(mcbs_batch* b, uint32_t* out, size_t row_words, hipStream_t st) {
    const uint64_t total = (uint64_t)b->S.E * b->def_pack.W;
    hipLaunchKernelGGL(defender_obs_packed_kernel, dim3((uint32_t)((total + 255u) / 256u)), dim3(256), 0, st, b->S, b->T, b->def_pack, out, row_words);
    return launch_ok("packed defender observation");
}

extern "C" int mcbs_defender_observe_packed(mcbs_batch* b, uint32_t* out, size_t row_words, void* stream) {
    if (!b || !out) return fail(MCBS_EINVAL, "null argument");
    MCBS_ON_DEVICE(b);
    if (const int rc = defender_packing_ok(b, "mcbs_defender_observe_packed", row_words)) return rc;
    if (const int rc = defender_live_rows_ok(b)) return rc;
    return launch_defender_obs_packed(b, out, row_words, (hipStream_t)stream);
}

// 32 rows per workgroup and pass (pack / unpack kernels), at most `cap` workgroups: the kernels loop over the rows beyond a grid's worth
static dim3 defender_rows_grid(uint64_t n_rows, uint64_t rows_per_block, uint32_t cap) {
    const uint64_t blocks = (n_rows + rows_per_block - 1u) / rows_per_block;
    return dim3(blocks < cap ? (uint32_t)blocks : cap);
}

extern "C" int mcbs_pack_defender_observation(const mcbs_batch* b, const mcbs_defender_obs* dense, uint64_t n_rows, uint32_t* out, size_t row_words,
                                              void* stream) {
    if (!b || !dense || !out) return fail(MCBS_EINVAL, "null argument");
    MCBS_ON_DEVICE(b);
    if (const int rc = defender_packing_ok(b, "mcbs_pack_defender_observation", row_words)) return rc;
    if (!defender_obs_complete(dense)) return fail(MCBS_EINVAL, "mcbs_pack_defender_observation: all four int8 fields are packed, one is NULL");
    if (n_rows == 0) return MCBS_OK;
    hipLaunchKernelGGL(pack_defender_obs_kernel, defender_rows_grid(n_rows, 32u, 16384u), dim3(256), 0, (hipStream_t)stream, b->def_pack, def_dense(dense),
                       n_rows, out, row_words);
    return launch_ok("pack defender observation");
}

extern "C" int mcbs_unpack_defender_observation(const mcbs_batch* b, const uint32_t* packed, size_t row_words, const int64_t* index,
                                                uint64_t n_source_rows, uint64_t n_rows, const mcbs_defender_obs* out, void* stream) {
    if (!b || !packed || !out) return fail(MCBS_EINVAL, "null argument");
    MCBS_ON_DEVICE(b);
    if (const int rc = defender_packing_ok(b, "mcbs_unpack_defender_observation", row_words)) return rc;
    if (!index && n_rows > n_source_rows) return fail(MCBS_EINVAL, "mcbs_unpack_defender_observation: %llu rows asked of %llu stored ones and no index",
                                                      (unsigned long long)n_rows, (unsigned long long)n_source_rows);
    if (n_rows == 0) return MCBS_OK;
    hipLaunchKernelGGL(unpack_defender_obs_kernel, defender_rows_grid(n_rows, 32u, 16384u), dim3(256), 0, (hipStream_t)stream, b->def_pack, packed, row_words,
                       index, n_source_rows, n_rows, def_dense<DefDenseOut>(out));
    return launch_ok("unpack defender observation");
}

extern "C" int mcbs_encode_defender_features(const mcbs_batch* b, const mcbs_defender_obs* dense, const uint32_t* packed, size_t row_words,
                                             const int64_t* index, uint64_t n_source_rows, uint64_t n_rows, void* out, size_t out_row_stride,
                                             int32_t dtype, int32_t* bad_rows, void* stream) {
    const char* who = "mcbs_encode_defender_features";
    if (!b || !out) return fail(MCBS_EINVAL, "null argument");
    MCBS_ON_DEVICE(b);
    if (!dense == !packed) return fail(MCBS_EINVAL, "%s: the source is either the dense fields or packed rows: exactly one of them", who);
    if (const int rc = defender_packing_ok(b, who, packed ? row_words : b->def_pack.W)) return rc;
    if (dense && !defender_obs_complete(dense)) return fail(MCBS_EINVAL, "%s: all four int8 fields are read, one is NULL", who);
    if (dtype != MCBS_FEATURES_F32 && dtype != MCBS_FEATURES_BF16 && dtype != MCBS_FEATURES_F16)
        return fail(MCBS_EINVAL, "features dtype must be MCBS_FEATURES_F32, MCBS_FEATURES_BF16 or MCBS_FEATURES_F16");
    const DefPackGeom& G = b->def_pack;
    if (out_row_stride < G.F) return fail(MCBS_EINVAL, "out_row_stride %zu is shorter than the %u feature columns", out_row_stride, G.F);
    if (!index && n_rows > n_source_rows) return fail(MCBS_EINVAL, "%s: %llu rows asked of %llu stored ones and no index", who,
                                                      (unsigned long long)n_rows, (unsigned long long)n_source_rows);
    if (n_rows == 0) return MCBS_OK;
    const DefDense src = dense ? def_dense(dense) : DefDense{};
    const size_t item = dtype == MCBS_FEATURES_F32 ? 4u : 2u;
    const uint32_t one = dtype == MCBS_FEATURES_F32 ? 0x3F800000u : dtype == MCBS_FEATURES_BF16 ? 0x3F80u : 0x3C00u;      // 1.0 as the dtype's pattern
    rows_dispatch<1u, 2u>(item, out, out_row_stride, [&](auto es, auto gw, auto vec) {
        using T = std::conditional_t<decltype(es)::value == 4u, uint32_t, uint16_t>;
        constexpr uint32_t GW = decltype(gw)::value;
        constexpr bool VEC = decltype(vec)::value;
        // rows per pass of a workgroup's 256 threads: as many whole rows of `ngroup` store groups as fit, at least one
        const uint32_t ngroup = (G.F + GW - 1u) / GW, RB = ngroup <= 256u ? 256u / ngroup : 1u;
        const dim3 grid = defender_rows_grid(n_rows, RB, 8192u);
        pick<0, 1>(packed ? 1 : 0, [&](auto pk) {
            hipLaunchKernelGGL((encode_defender_features_kernel<T, GW, VEC, decltype(pk)::value != 0>), grid, dim3(256), 0, (hipStream_t)stream, G, src, packed,
                               row_words, index, n_source_rows, n_rows, static_cast<T*>(out), out_row_stride, (T)one, ngroup, RB, fast_div_host(ngroup), bad_rows);
        });
    });
    return launch_ok("encode defender features");
}

// 1: the turn launch writes the packed rows itself; 2: the turn, then the kernel of mcbs_defender_observe_packed
extern "C" int32_t mcbs_defender_wrapper_step_packed_launches(const mcbs_batch* b) {
    if (!b || b->cfg.defender_kind != MCBS_DEFENDER_EXTERNAL) return 0;
    return b->variant.fused_defender_obs ? 1 : 2;
}

extern "C" int mcbs_defender_wrapper_step_packed(mcbs_batch* b, const int64_t* actions, uint32_t* packed_out, size_t row_words,
                                                 const mcbs_defender_wrapper_buffers* w, const mcbs_defender_wrapper_cfg* cfg, void* stream) {
    if (!b || !actions || !packed_out || !w || !cfg) return fail(MCBS_EINVAL, "null argument");
    MCBS_ON_DEVICE(b);
    if (const int rc = defender_packing_ok(b, "mcbs_defender_wrapper_step_packed", row_words)) return rc;
    if (const int rc = defender_live_rows_ok(b)) return rc;
    if (!arrays_set(w, 0)) return fail(MCBS_EINVAL, "mcbs_defender_wrapper_buffers: every array is required");
    hipStream_t st = (hipStream_t)stream;
    const bool fused = b->variant.fused_defender_obs && reinterpret_cast<uintptr_t>(packed_out) % 16 == 0;
    if (fused)
        return launch_defender_turn(b, nullptr, st, "defender turn + reward shaping + packed observation", [&](auto wt, dim3 grid, dim3 block, const DefObs&) {
            hipLaunchKernelGGL((defender_turn_post_packed_kernel<decltype(wt)::value>), grid, block, 0, st, b->S, b->T, b->C_dev, actions, *w, *cfg, b->def_pack,
                               packed_out, row_words);
        });
    const int rc = launch_defender_turn(b, nullptr, st, "defender turn + reward shaping", [&](auto wt, dim3 grid, dim3 block, const DefObs& dob) {
        hipLaunchKernelGGL((defender_turn_post_kernel<decltype(wt)::value>), grid, block, 0, st, b->S, b->T, b->C_dev, actions, *w, *cfg, dob);
    });
    if (rc) return rc;
    return launch_defender_obs_packed(b, packed_out, row_words, st);
}

// ------------------------------------------------------------------ the two-agent turn (mcbs_two_agent.hip)
// the batch-level half of mcbs_two_agent_step's scope: -> nullptr when the batch fits, else the reason
static const char* two_agent_batch_reason(const mcbs_batch* b) {
    if (b->cfg.defender_kind != MCBS_DEFENDER_EXTERNAL) return "batch was not created with MCBS_DEFENDER_EXTERNAL";
    if (!b->variant.fused_wrapper) return "the attacker's wrapper step of this batch is not one launch (packed batch, at most 16 nodes and cached credentials)";
    if (!b->variant.fused_defender_obs || b->S.WT != 1u) return "the defender's turn of this batch cannot write its own observation";
    return nullptr;
}

extern "C" int32_t mcbs_two_agent_step_launches(const mcbs_batch* b) {
    return (b && !two_agent_batch_reason(b)) ? 1 : 0;
}

extern "C" int mcbs_two_agent_step(mcbs_batch* b, const int64_t* multidiscrete, const int64_t* discrete, int32_t* decoded, const mcbs_info_buffers* info,
                                   const mcbs_obs_buffers* obs, const mcbs_wrapper_buffers* w, float modifier, int32_t attacker_max_timesteps,
                                   const int64_t* defender_actions, const mcbs_defender_obs* defender_obs, const mcbs_defender_wrapper_buffers* dw,
                                   const mcbs_defender_wrapper_cfg* dcfg, const mcbs_episode_buffers* ep, void* stream) {
    if (!b || !w || !decoded || !obs || !defender_actions || !defender_obs || !dw || !dcfg) return fail(MCBS_EINVAL, "null argument");
    MCBS_ON_DEVICE(b);
    // every check before the launch: a refused call launches nothing and changes no state
    if (const char* why = two_agent_batch_reason(b)) return fail(MCBS_EINVAL, "two-agent turn: %s", why);
    StepIO io;
    if (const int rc = attacker_turn_io(b, multidiscrete, discrete, decoded, info, w, modifier, attacker_max_timesteps, 0, nullptr, nullptr, &io)) return rc;
    if (!arrays_set(dw, 0)) return fail(MCBS_EINVAL, "mcbs_defender_wrapper_buffers: every array is required");
    if (ep && !arrays_set(ep, 0)) return fail(MCBS_EINVAL, "mcbs_episode_buffers: every array is required");
    TwoAgentArgs D{};
    D.actions = defender_actions; D.dw = *dw; D.dcfg = *dcfg;
    D.obs = fused_defender_obs(b, defender_obs);
    if (!D.obs.fused) return fail(MCBS_EINVAL, "two-agent turn: the defender's observation arrays must lie on 16-byte boundaries");
    if (ep) D.ep = *ep;
    FusedArgs A;
    if (!fused_wrapper_args(b, multidiscrete, discrete, decoded, obs, w, modifier, attacker_max_timesteps, 0, nullptr, nullptr, &A))
        return fail(MCBS_EINVAL, "two-agent turn: the attacker's request is outside the one-launch wrapper step (a mask field, or an observation "
                                 "array that is not on a 16-byte boundary)");
    b->all_fresh = false;
    hipLaunchKernelGGL(two_agent_kernel, dim3((b->S.E + 63u) / 64u), dim3(FUSED_THREADS), 0, (hipStream_t)stream, b->S, b->T, b->C_dev, io, A, D);
    return turn_launched(b, "two-agent turn");
}

// ---- the training turn: both auto-resets and the reset_request hand-shake in the same launch (two_agent_train_kernel)
extern "C" int32_t mcbs_two_agent_train_step_launches(const mcbs_batch* b) {
    return (b && !two_agent_batch_reason(b)) ? 1 : 0;
}

extern "C" int mcbs_two_agent_train_step(mcbs_batch* b, const int64_t* multidiscrete, const int64_t* discrete, int32_t* decoded, const mcbs_info_buffers* info,
                                         const mcbs_obs_buffers* obs, const mcbs_wrapper_buffers* w, float modifier, int32_t attacker_max_timesteps,
                                         const mcbs_row_copies* keep, const mcbs_row_copies* fresh, const int64_t* defender_actions,
                                         const mcbs_defender_obs* defender_obs, const mcbs_defender_wrapper_buffers* dw,
                                         const mcbs_defender_wrapper_cfg* dcfg, const mcbs_training_buffers* tr, void* stream) {
    const char* who = "two-agent training turn";
    if (!b || !w || !decoded || !obs || !keep || !fresh || !defender_actions || !defender_obs || !dw || !dcfg || !tr) return fail(MCBS_EINVAL, "null argument");
    MCBS_ON_DEVICE(b);
    // every check before the launch: a refused call launches nothing and changes no state
    if (const char* why = two_agent_batch_reason(b)) return fail(MCBS_EINVAL, "%s: %s", who, why);
    StepIO io;
    if (const int rc = attacker_turn_io(b, multidiscrete, discrete, decoded, info, w, modifier, attacker_max_timesteps, 1, keep, fresh, &io)) return rc;
    if (!arrays_set(dw, 0)) return fail(MCBS_EINVAL, "mcbs_defender_wrapper_buffers: every array is required");
    if (!arrays_set(tr, 0)) return fail(MCBS_EINVAL, "mcbs_training_buffers: every array is required");
    if (!defender_obs_complete(defender_obs)) return fail(MCBS_EINVAL, "%s: every field of the defender's observation is required", who);
    TrainArgs D{};
    D.actions = defender_actions; D.dw = *dw; D.dcfg = *dcfg;
    D.obs = fused_defender_obs(b, defender_obs);
    const mcbs_defender_obs terminal{tr->terminal_infected_nodes, tr->terminal_incoming_firewall_status, tr->terminal_outgoing_firewall_status,
                                     tr->terminal_services_status};
    D.term = fused_defender_obs(b, &terminal);
    if (!D.obs.fused || !D.term.fused)
        return fail(MCBS_EINVAL, "%s: the defender's live and terminal observation arrays must lie on 16-byte boundaries", who);
    D.fresh_infected = tr->fresh_infected_nodes; D.fresh_fw_in = tr->fresh_incoming_firewall_status; D.fresh_fw_out = tr->fresh_outgoing_firewall_status;
    D.request = tr->attacker_reset_request; D.dreturn = tr->defender_return;
    D.a_valid_out = tr->attacker_valid_out; D.a_invalid_out = tr->attacker_invalid_out;
    D.d_return_out = tr->defender_return_out; D.d_length_out = tr->defender_length_out;
    D.d_valid_out = tr->defender_valid_out; D.d_invalid_out = tr->defender_invalid_out; D.d_dones = tr->defender_dones;
    FusedArgs A;
    if (!fused_wrapper_args(b, multidiscrete, discrete, decoded, obs, w, modifier, attacker_max_timesteps, 1, keep, fresh, &A))
        return fail(MCBS_EINVAL, "%s: the attacker's request is outside the one-launch wrapper step (a mask field, an observation array that is "
                                 "not on a 16-byte boundary, or a field without its terminal array in `keep` and its reset row in `fresh`)", who);
    // no array this launch writes may share a byte with another array it reads or writes
    const uint64_t E = b->S.E, N = b->S.N, Sv = b->C.n_services;
    Extents ext;
    ext.bytes("decoded", decoded, E * 20u, true); ext.bytes("multidiscrete", multidiscrete, E * 80u, false);
    ext.bytes("discrete", discrete, E * 8u, false); ext.bytes("defender_actions", defender_actions, E * 96u, false);
    static_assert(FUSED_FIELDS == 5, "kObsFields names the fused step's fields");
    for (uint32_t f = 0; f < FUSED_FIELDS; ++f) {
        ext.bytes(kObsFields[f], A.obs[f], E * 4u * A.dwords[f], true);
        ext.bytes("a terminal observation array (keep)", A.obs[f] ? A.term[f] : nullptr, E * 4u * A.dwords[f], true);
        ext.bytes("a reset row (fresh)", A.obs[f] ? A.fresh[f] : nullptr, 4ull * A.dwords[f], false);
    }
    add_arrays(ext, "w->", w, kWrapperArrays, E, N, Sv, true);
    add_arrays(ext, "info->", info, kInfoArrays, E, N, Sv, true);
    add_arrays(ext, "defender_obs->", defender_obs, kDefenderObsArrays, E, N, Sv, true);
    add_arrays(ext, "dw->", dw, kDefenderWrapperArrays, E, N, Sv, true);
    add_arrays(ext, "tr->", tr, kTrainingArrays, E, N, Sv, true);
    if (const int rc = disjoint(who, ext)) return rc;
    b->all_fresh = false;
    hipLaunchKernelGGL(two_agent_train_kernel, dim3((b->S.E + 63u) / 64u), dim3(FUSED_THREADS), 0, (hipStream_t)stream, b->S, b->T, b->C_dev, io, A, D);
    return turn_launched(b, "two-agent training turn", true);      // (the digests it wrote carry their observation's discovery order)
}

// ---- the training turn with both observations as packed rows (two_agent_train_packed_kernel): no multi-launch form, no mixed form
// the packed step's LDS room for a row of this packing (mcbs_wrapper_fused.hip FusedPackedStore)
static bool packed_step_room(const mcbs_obs_packing* p) {
    return p->P.W <= FUSED_PACKED_MAX_WORDS && p->P.W + 1u + p->P.V <= FUSED_PACKED_TABLE_DWORDS;
}

extern "C" int32_t mcbs_two_agent_train_step_packed_launches(const mcbs_batch* b, const mcbs_obs_packing* p) {
    return (b && p && !two_agent_batch_reason(b) && obs_packing_fits(b, p) && packed_step_room(p) && b->def_pack.W <= DEF_WMAX) ? 1 : 0;
}

extern "C" int mcbs_two_agent_train_step_packed(mcbs_batch* b, const int64_t* multidiscrete, const int64_t* discrete, int32_t* decoded,
                                                const mcbs_info_buffers* info, const mcbs_obs_packing* p, uint32_t* packed, uint32_t* packed_terminal,
                                                const uint32_t* packed_fresh, size_t row_words, const mcbs_wrapper_buffers* w, float modifier,
                                                int32_t attacker_max_timesteps, const int64_t* defender_actions, uint32_t* defender_packed,
                                                size_t defender_row_words, const mcbs_defender_wrapper_buffers* dw, const mcbs_defender_wrapper_cfg* dcfg,
                                                const mcbs_training_packed_buffers* tr, void* stream) {
    const char* who = "two-agent training turn (packed rows)";
    if (!b || !w || !decoded || !p || !packed || !packed_terminal || !packed_fresh || !defender_actions || !defender_packed || !dw || !dcfg || !tr)
        return fail(MCBS_EINVAL, "null argument");
    MCBS_ON_DEVICE(b);
    // every check before the launch: a refused call launches nothing and changes no state
    if (const char* why = two_agent_batch_reason(b)) return fail(MCBS_EINVAL, "%s: %s", who, why);
    StepIO io;
    if (const int rc = attacker_turn_io(b, multidiscrete, discrete, decoded, info, w, modifier, attacker_max_timesteps, 1, nullptr, nullptr, &io)) return rc;
    if (!arrays_set(dw, 0)) return fail(MCBS_EINVAL, "mcbs_defender_wrapper_buffers: every array is required");
    if (!arrays_set(tr, 0)) return fail(MCBS_EINVAL, "mcbs_training_packed_buffers: every array is required");
    if (!obs_packing_fits(b, p)) return fail(MCBS_EINVAL, "%s: the packing was created for a batch of another device or geometry", who);
    const uint32_t W = p->P.W, V = p->P.V, Wd = b->def_pack.W;
    if (row_words < W) return fail(MCBS_EINVAL, "%s: row_words %zu is shorter than the %u words of a packed row", who, row_words, W);
    if (!packed_step_room(p))
        return fail(MCBS_EINVAL, "%s: a packed row of %u words and %u values is beyond the LDS room the step keeps for the fresh row (%u words) and "
                                 "its tables (%u entries)", who, W, V, FUSED_PACKED_MAX_WORDS, FUSED_PACKED_TABLE_DWORDS);
    if (const int rc = defender_packing_ok(b, who, defender_row_words)) return rc;
    if (Wd > DEF_WMAX) return fail(MCBS_EINVAL, "%s: a packed defender row of %u words is beyond the %u the turn writes itself", who, Wd, DEF_WMAX);
    if (reinterpret_cast<uintptr_t>(defender_packed) % 16u || reinterpret_cast<uintptr_t>(tr->terminal_defender_packed) % 16u)
        return fail(MCBS_EINVAL, "%s: defender_packed and tr->terminal_defender_packed must lie on 16-byte boundaries", who);
    if (defender_row_words != Wd && defender_row_words % 4u)
        return fail(MCBS_EINVAL, "%s: defender_row_words %zu is neither the %u words of a packed defender row nor a multiple of 4 (16-byte stores)",
                    who, defender_row_words, Wd);
    // no array this launch writes may share a byte with another array it reads or writes
    const uint64_t E = b->S.E;
    Extents ext;
    ext.bytes("decoded", decoded, E * 20u, true); ext.bytes("multidiscrete", multidiscrete, E * 80u, false);
    ext.bytes("discrete", discrete, E * 8u, false); ext.bytes("defender_actions", defender_actions, E * 96u, false);
    ext.rows("packed", packed, E, row_words, W, 4u, true); ext.rows("packed_terminal", packed_terminal, E, row_words, W, 4u, true);
    ext.bytes("packed_fresh", packed_fresh, (uint64_t)W * 4u, false);
    ext.rows("defender_packed", defender_packed, E, defender_row_words, Wd, 4u, true);
    ext.rows("tr->terminal_defender_packed", tr->terminal_defender_packed, E, defender_row_words, Wd, 4u, true);
    ext.bytes("tr->fresh_defender_packed", tr->fresh_defender_packed, (uint64_t)Wd * 4u, false);
    add_arrays(ext, "w->", w, kWrapperArrays, E, 0u, 0u, true);
    add_arrays(ext, "info->", info, kInfoArrays, E, 0u, 0u, true);
    add_arrays(ext, "dw->", dw, kDefenderWrapperArrays, E, 0u, 0u, true);
    add_arrays(ext, "tr->", tr, kTrainingPackedArrays, E, 0u, 0u, true);
    if (const int rc = disjoint(who, ext)) return rc;
    const mcbs_obs_buffers none{};
    FusedArgs A;
    if (!fused_wrapper_args(b, multidiscrete, discrete, decoded, &none, w, modifier, attacker_max_timesteps, 1, nullptr, nullptr, &A))
        return fail(MCBS_EINVAL, "%s: the wrapper step of this batch is not one launch", who);
    FusedPackedArgs PA{};
    PA.packed = packed; PA.term = packed_terminal; PA.fresh = packed_fresh; PA.desc = p->desc_dev; PA.word_first = p->word_first_dev;
    PA.row_words = row_words; PA.W = W; PA.V = V;
    PA.off1 = p->P.off[1]; PA.off2 = p->P.off[2]; PA.off3 = p->P.off[3]; PA.off4 = p->P.off[4];
    TrainPackedArgs D{};
    D.actions = defender_actions; D.dw = *dw; D.dcfg = *dcfg; D.W = Wd;
    TrainPackedStoreArgs Q{};
    Q.G = b->def_pack; Q.packed = defender_packed; Q.term = tr->terminal_defender_packed; Q.fresh = tr->fresh_defender_packed;
    Q.row_words = defender_row_words;
    D.request = tr->attacker_reset_request; D.dreturn = tr->defender_return;
    D.a_valid_out = tr->attacker_valid_out; D.a_invalid_out = tr->attacker_invalid_out;
    D.d_return_out = tr->defender_return_out; D.d_length_out = tr->defender_length_out;
    D.d_valid_out = tr->defender_valid_out; D.d_invalid_out = tr->defender_invalid_out; D.d_dones = tr->defender_dones;
    b->all_fresh = false;
    hipLaunchKernelGGL(two_agent_train_packed_kernel, dim3((b->S.E + 63u) / 64u), dim3(FUSED_THREADS), 0, (hipStream_t)stream, b->S, b->T, b->C_dev, io, A, PA, D, Q);
    return turn_launched(b, "two-agent training turn (packed rows)", true);      // (the digests it wrote carry their observation's discovery order)
}

// ------------------------------------------------------------------ state export / import (debug, synchronous)
extern "C" size_t mcbs_state_record_bytes(const mcbs_batch* b) {
    if (!b) return 0;
    const size_t n = sizeof(mcbs_state_header) + sizeof(mcbs_state_node) * b->S.N + 2ull * b->S.N + 2ull * b->cfg.maximum_total_credentials;
    return align_up(n, 16);
}

extern "C" int mcbs_get_state(mcbs_batch* b, void* host_buf, size_t nbytes) {
    if (!b || !host_buf) return fail(MCBS_EINVAL, "null argument");
    const size_t rb = mcbs_state_record_bytes(b);
    const DevState& S = b->S;
    if (nbytes < rb * S.E) return fail(MCBS_EINVAL, "state buffer too small: need %zu bytes", rb * S.E);
    DeviceGuard guard(b->cfg.device);
    HIP_TRY(guard.err);
    HIP_TRY(hipDeviceSynchronize());
    std::vector<uint8_t> host(b->arena_bytes);
    HIP_TRY(hipMemcpy(host.data(), b->arena, b->arena_bytes, hipMemcpyDeviceToHost));
    auto at = [&](const void* devptr) { return host.data() + (static_cast<const uint8_t*>(devptr) - b->arena); };
    const uint4* h0 = reinterpret_cast<const uint4*>(at(S.h0));
    const double2* h1 = reinterpret_cast<const double2*>(at(S.h1));
    const uint32_t* ep = reinterpret_cast<const uint32_t*>(at(S.episode));
    const void* mk = at(S.masks);
    auto has = [&](int k, uint32_t n, uint32_t e) { return ((S.set_word(mk, k, n >> 6, e) >> (n & 63u)) & 1ull) != 0; };
    (void)has;
    const uint64_t* ring = S.ring ? reinterpret_cast<const uint64_t*>(at(S.ring)) : nullptr;
    const uint8_t* body = at(S.body);
    memset(host_buf, 0, rb * S.E);
    for (uint32_t e = 0; e < S.E; ++e) {
        uint8_t* p = static_cast<uint8_t*>(host_buf) + rb * e;
        mcbs_state_header* sh = reinterpret_cast<mcbs_state_header*>(p);
        const uint32_t flags = h0[e].y;
        sh->step_count = h0[e].x; sh->done = flags & F_DONE ? 1 : 0; sh->truncated = flags & F_TRUNC ? 1 : 0; sh->episode = ep[e];
        sh->n_discovered = h0[e].z & 0xFFFFu; sh->n_creds = h0[e].z >> 16;
        sh->last_outcome_kind = (flags >> F_KIND_SHIFT) & 0xFu; sh->last_escalation = (flags >> F_LEVEL_SHIFT) & 3u;
        sh->last_new_nodes = (flags >> F_NEWNODES_SHIFT) & 0x3FFu; sh->last_new_creds = (flags >> F_NEWCREDS_SHIFT) & 0x3FFu;
        sh->last_oob = flags & F_OOB ? 1 : 0;
        sh->cum_reward = h1[e].x; sh->availability = h1[e].y;
        mcbs_state_node* sn = reinterpret_cast<mcbs_state_node*>(p + sizeof(mcbs_state_header));
        const uint8_t* eb = body + (size_t)e * S.body_stride;
        for (uint32_t n = 0; n < S.N; ++n) {
            const Row r = S.row_get(eb, n);
            const uint64_t bit = 1ull << (n & 63u);
            sn[n].discovered_props = r.props_tags & ROW_PROPS_MASK; sn[n].attacked_ever = r.ever; sn[n].attacked_since = r.since;
            sn[n].discovered = has(M_DISC, n, e); sn[n].installed = has(M_INST, n, e);
            sn[n].ever_owned = has(M_EVER, n, e); sn[n].running = has(M_RUN, n, e);
            sn[n].privilege = (uint8_t)((has(M_PLO, n, e) ? 1 : 0) | (has(M_PHI, n, e) ? 2 : 0));
            sn[n].tags = (uint8_t)(r.props_tags >> 60);
            sn[n].countdown = 0;
            if (!sn[n].running && ring) {   // remaining steps = distance from the defender clock to the node's ring slot
                const uint32_t d = (h0[e].w >> 16) & 15u;
                for (uint32_t s = 0; s < 16u; ++s)
                    if (ring[((size_t)s * S.WT + (n >> 6)) * S.E + e] & bit) sn[n].countdown = (uint8_t)((s + 16u - d) & 15u);
            }
        }
        uint16_t* order = reinterpret_cast<uint16_t*>(p + sizeof(mcbs_state_header) + sizeof(mcbs_state_node) * S.N);
        for (uint32_t k = 0; k < S.N; ++k) order[k] = k < sh->n_discovered ? (uint16_t)S.disc_get(mk, eb, e, k) : 0xFFFF;
        uint16_t* cc = order + S.N;
        for (uint32_t k = 0; k < b->cfg.maximum_total_credentials; ++k) cc[k] = k < sh->n_creds ? (uint16_t)S.cred_get(mk, eb, e, k) : 0xFFFF;
    }
    return MCBS_OK;
}

extern "C" int mcbs_set_state(mcbs_batch* b, const void* host_buf, size_t nbytes) {
    if (!b || !host_buf) return fail(MCBS_EINVAL, "null argument");
    const size_t rb = mcbs_state_record_bytes(b);
    const DevState& S = b->S;
    if (nbytes < rb * S.E) return fail(MCBS_EINVAL, "state buffer too small: need %zu bytes", rb * S.E);
    const mcbs_topo_header* th = b->topo->H();
    DeviceGuard guard(b->cfg.device);
    HIP_TRY(guard.err);
    HIP_TRY(hipDeviceSynchronize());
    std::vector<uint8_t> host(b->arena_bytes);
    HIP_TRY(hipMemcpy(host.data(), b->arena, b->arena_bytes, hipMemcpyDeviceToHost));   // keeps init image, digest, episode
    auto at = [&](const void* devptr) { return host.data() + (static_cast<const uint8_t*>(devptr) - b->arena); };
    uint4* h0 = reinterpret_cast<uint4*>(at(S.h0));
    double2* h1 = reinterpret_cast<double2*>(at(S.h1));
    uint32_t* ep = reinterpret_cast<uint32_t*>(at(S.episode));
    void* mk = at(S.masks);
    uint64_t* cach_h = S.wide ? reinterpret_cast<uint64_t*>(at(S.cach)) : nullptr;
    auto add = [&](int k, uint32_t n, uint32_t e) {
        if (cach_h && k == M_CACH) cach_h[(size_t)(n >> 6) * S.E + e] |= 1ull << (n & 63u);
        else S.put_word(mk, k, n >> 6, e, S.set_word(mk, k, n >> 6, e) | (1ull << (n & 63u)));
    };
    uint64_t* ring = S.ring ? reinterpret_cast<uint64_t*>(at(S.ring)) : nullptr;
    uint8_t* body = at(S.body);
    const mcbs_triple* tr = reinterpret_cast<const mcbs_triple*>(b->topo->host.data() + th->off_triple);
    for (uint32_t e = 0; e < S.E; ++e) {
        const uint8_t* p = static_cast<const uint8_t*>(host_buf) + rb * e;
        const mcbs_state_header* sh = reinterpret_cast<const mcbs_state_header*>(p);
        const mcbs_state_node* sn = reinterpret_cast<const mcbs_state_node*>(p + sizeof(mcbs_state_header));
        const uint16_t* order = reinterpret_cast<const uint16_t*>(p + sizeof(mcbs_state_header) + sizeof(mcbs_state_node) * S.N);
        const uint16_t* cc = order + S.N;
        if (sh->n_discovered > S.N || sh->n_creds > th->n_triples) return fail(MCBS_EINVAL, "env %u: list lengths out of range", e);
        for (uint32_t w = 0; w < S.WT; ++w) {
            for (int k = 0; k < M_COUNT; ++k) S.put_word(mk, k, w, e, 0ull);
            if (cach_h && w == 0) for (uint32_t cw = 0; cw < S.TW; ++cw) cach_h[(size_t)cw * S.E + e] = 0ull;
            if (ring) for (uint32_t s = 0; s < 16u; ++s) ring[((size_t)s * S.WT + w) * S.E + e] = 0;
        }
        uint8_t* eb = body + (size_t)e * S.body_stride;
        if (b->cfg.defender_kind == MCBS_DEFENDER_RANDOM_EVENTS) {   // the canonical record does not carry the random-events overlay
            const uint8_t* init = at(S.init_body);                   // (vulnerability keys, service bits, rule lists): back to the
            memcpy(eb + b->C.ere_off_present, init + b->C.ere_off_present, S.body_stride - b->C.ere_off_present);   // topology's initial ones
        }
        uint32_t owned = 0;
        const uint32_t dclk = h0[e].w >> 16;      // the defender clock is not part of the canonical record: keep the current phase
        for (uint32_t n = 0; n < S.N; ++n) {
            const uint64_t bit = 1ull << (n & 63u);
            if (sn[n].privilege > 3 || sn[n].countdown > 15) return fail(MCBS_EINVAL, "env %u node %u: bad privilege / countdown", e, n);
            if (sn[n].discovered) add(M_DISC, n, e);
            if (sn[n].installed) add(M_INST, n, e);
            if (sn[n].ever_owned) add(M_EVER, n, e);
            if (sn[n].running) add(M_RUN, n, e);
            if (sn[n].privilege & 1) add(M_PLO, n, e);
            if (sn[n].privilege & 2) add(M_PHI, n, e);
            owned += sn[n].privilege >= 1;
            if (!sn[n].running && ring) ring[((size_t)((dclk + sn[n].countdown) & 15u) * S.WT + (n >> 6)) * S.E + e] |= bit;
            Row r{};
            r.props_tags = (sn[n].discovered_props & ROW_PROPS_MASK) | ((uint64_t)(sn[n].tags & 0xFu) << 60);
            r.ever = sn[n].attacked_ever; r.since = sn[n].attacked_since;
            S.row_put(eb, n, r);
        }
        if (S.packed) static_cast<uint4*>(mk)[(size_t)S.E + e] = make_uint4(0u, 0u, 0u, 0u);   // the lists word: zero at and past the counts
        for (uint32_t i = 0; i < sh->n_discovered; ++i) {
            if (order[i] >= S.N) return fail(MCBS_EINVAL, "env %u: discovery order entry out of range", e);
            S.disc_put(mk, eb, e, i, order[i]);
        }
        for (uint32_t i = 0; i < sh->n_creds; ++i) {
            if (cc[i] >= th->n_triples) return fail(MCBS_EINVAL, "env %u: credential cache entry out of range", e);
            S.cred_put(mk, eb, e, i, cc[i]);
            add(M_CACH, cc[i], e);
            const uint32_t c = tr[cc[i]].cred;                     // a cached triple implies its credential string is gathered
            add(M_GATH, c, e);
        }
        const uint32_t flags = (sh->done ? F_DONE : 0u) | (sh->truncated ? F_TRUNC : 0u) | (sh->last_oob ? F_OOB : 0u) |
                               ((sh->last_outcome_kind & 0xFu) << F_KIND_SHIFT) | ((sh->last_escalation & 3u) << F_LEVEL_SHIFT) |
                               ((sh->last_new_nodes & 0x3FFu) << F_NEWNODES_SHIFT) | ((sh->last_new_creds & 0x3FFu) << F_NEWCREDS_SHIFT);
        h0[e] = make_uint4(sh->step_count, flags, sh->n_discovered | (sh->n_creds << 16), owned | (dclk << 16));
        h1[e] = make_double2(sh->cum_reward, sh->availability);
        ep[e] = sh->episode;
    }
    HIP_TRY(hipMemcpy(b->arena, host.data(), b->arena_bytes, hipMemcpyHostToDevice));
    b->all_fresh = false;
    b->digest_state = 0;
    return MCBS_OK;
}

// diagnostic builds (-DMCBS_DIAG): per-wavefront s_memtime stamps of the next step launches; not part of the public ABI
extern "C" int mcbs_diag_set_stamps(mcbs_batch* b, unsigned long long* dev_buf) {
    if (!b) return fail(MCBS_EINVAL, "null batch");
    b->stamps = dev_buf;
    return MCBS_OK;
}

// ------------------------------------------------------------------ timing
extern "C" int mcbs_timing_enable(mcbs_batch* b, int32_t on) {
    if (!b) return fail(MCBS_EINVAL, "null batch");
    b->timing = on != 0;
    b->ev_used = 0; b->timed_ms = 0.0; b->timed_launches = 0;
    return MCBS_OK;
}

extern "C" int mcbs_timing_read(mcbs_batch* b, double* total_ms, uint64_t* launches) {
    if (!b) return fail(MCBS_EINVAL, "null batch");
    MCBS_ON_DEVICE(b);
    for (size_t i = 0; i + 1 < b->ev_used; i += 2) {
        HIP_TRY(hipEventSynchronize(b->ev[i + 1]));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, b->ev[i], b->ev[i + 1]));
        b->timed_ms += ms;
        b->timed_launches += 1;
    }
    b->ev_used = 0;
    if (total_ms) *total_ms = b->timed_ms;
    if (launches) *launches = b->timed_launches;
    return MCBS_OK;
}
