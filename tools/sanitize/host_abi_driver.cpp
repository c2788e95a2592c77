// Host-only exercise of libnmz_gpu's C ABI under ASan/UBSan (build/host_abi_asan) and TSan (build/host_abi_tsan),
// on a machine without a GPU: argument validation of every entry point, parameter resolution
// (randompolicy.go:223-225,337-339, util/queue/impl.go:36-38), the thread-local error message, and context
// opening failing cleanly when no device is present. Exit status 0 = every check held.
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/nmz_gpu.h"
#include "../../namazu_amd/csrc/scratch_layout.h"

static std::atomic<int> g_fail{0};
#define CHECK(c)                                                                   \
    do {                                                                           \
        if (!(c)) {                                                                \
            std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
            g_fail++;                                                              \
        }                                                                          \
    } while (0)

static void params_cases() {
    nmz_random_params p;
    CHECK(nmz_random_params_resolve(30000000, 100000000, 0.1, &p) == NMZ_OK);
    CHECK(p.min_ns[1] == 24000000 && p.max_ns[1] == 80000000 && p.fault_threshold == 100);
    CHECK(nmz_random_params_resolve(5, 5, 1.0, &p) == NMZ_OK && p.fault_threshold == 1000);
    CHECK(nmz_random_params_resolve(1, 3, 0.999, &p) == NMZ_OK && p.fault_threshold == 999);
    CHECK(nmz_random_params_resolve(-7, 7, 0.0, &p) == NMZ_OK && p.min_ns[1] == -5 && p.max_ns[1] == 5);
    CHECK(nmz_random_params_resolve(INT64_MIN, INT64_MAX, 0.5, &p) == NMZ_OK);
    CHECK(nmz_random_params_resolve(10, 5, 0.1, &p) == NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "minDuration") != nullptr);
    CHECK(nmz_random_params_resolve(0, 1, -0.01, &p) == NMZ_EINVAL);
    CHECK(nmz_random_params_resolve(0, 1, 1.01, &p) == NMZ_EINVAL);
    CHECK(nmz_random_params_resolve(0, 1, std::nan(""), &p) == NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "faultActionProbability") != nullptr);
    CHECK(nmz_random_params_resolve(0, 1, 0.5, nullptr) == NMZ_EINVAL);
}

static void null_ctx_cases() {
    uint32_t off[2] = {0, 1};
    uint8_t b[1] = {'x'};
    uint64_t o64[2] = {0, 1}, s64[1] = {7}, keys[8], sig[2];
    uint32_t u32[8];
    int64_t d64[4];
    uint8_t f8[4];
    nmz_sched_stats st[2];
    nmz_topk_entry tk[2];
    nmz_random_params rp;
    nmz_random_params_resolve(1, 2, 0.5, &rp);
    CHECK(nmz_replayable_sweep(nullptr, off, b, 1, off, b, 1, 10, st, nullptr, 0, 0, nullptr) == NMZ_EINVAL);
    CHECK(nmz_replayable_plan_create(nullptr, off, b, 1, 10, 1, nullptr) == NMZ_EINVAL);
    CHECK(nmz_replayable_sweep_dev(nullptr, off, b, 1, st, nullptr) == NMZ_EINVAL);
    CHECK(nmz_replayable_sweep_topk_dev(nullptr, off, b, 1, 0, 1, st, tk, nullptr) == NMZ_EINVAL);
    CHECK(nmz_replayable_decide(nullptr, b, 1, off, b, 1, 10, d64) == NMZ_EINVAL);
    CHECK(nmz_random_sweep(nullptr, 0, 1, s64, f8, 1, &rp, st, nullptr, nullptr, 0, 0, nullptr) == NMZ_EINVAL);
    CHECK(nmz_random_plan_create(nullptr, s64, f8, 1, &rp, 1, nullptr) == NMZ_EINVAL);
    CHECK(nmz_random_sweep_dev(nullptr, 0, 1, st, nullptr) == NMZ_EINVAL);
    CHECK(nmz_random_decide(nullptr, 1, s64, f8, 1, &rp, d64, f8) == NMZ_EINVAL);
    CHECK(nmz_topk_select_dev(nullptr, st, 1, 0, 1, tk, nullptr) == NMZ_EINVAL);
    CHECK(nmz_ed_pairs(nullptr, o64, s64, 1, u32, 1, 0, u32) == NMZ_EINVAL);
    CHECK(nmz_ed_allpairs_knn(nullptr, o64, s64, 1, 8, 1, u32, u32) == NMZ_EINVAL);
    CHECK(nmz_ed_plan_create(nullptr, o64, s64, 1, 8, nullptr) == NMZ_EINVAL);
    CHECK(nmz_ed_allpairs_knn_dev(nullptr, 1, keys, nullptr) == NMZ_EINVAL);
    CHECK(nmz_ed_allpairs_knn_shard_dev(nullptr, 1, 0, 1, keys, nullptr) == NMZ_EINVAL);
    CHECK(nmz_knn_merge_dev(nullptr, keys, 1, 1, 1, keys, nullptr) == NMZ_EINVAL);
    CHECK(nmz_ed_plan_counters(nullptr, keys, nullptr) == NMZ_EINVAL);
    CHECK(nmz_trace_signatures(nullptr, o64, s64, nullptr, 1, sig) == NMZ_EINVAL);
    CHECK(nmz_unique_traces(nullptr, o64, s64, nullptr, 1, u32) == NMZ_EINVAL);
    CHECK(nmz_unique_traces_dev(nullptr, o64, s64, nullptr, 1, 0, sig, u32, nullptr) == NMZ_EINVAL);
    // decreasing offsets are refused before the context is looked at (the last pair, the first pair)
    uint64_t dec[4] = {0, 1, 1, 0}, dec0[3] = {1, 0, 1}, sig6[6];
    CHECK(nmz_trace_signatures(nullptr, dec, s64, nullptr, 3, sig6) == NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "offsets must be non-decreasing") != nullptr);
    CHECK(nmz_unique_traces(nullptr, dec0, s64, nullptr, 2, u32) == NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "offsets must be non-decreasing") != nullptr);
    CHECK(nmz_trace_signatures(nullptr, o64, s64, nullptr, 1, sig) == NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "ctx is NULL") != nullptr);
    CHECK(nmz_timing_enable(nullptr, 1) == NMZ_EINVAL);
    double ms;
    uint64_t cnt;
    CHECK(nmz_timing_read(nullptr, "x", &ms, &cnt, 0) == NMZ_EINVAL);
    CHECK(nmz_ed_plan_is_fast(nullptr) == 0);
    CHECK(nmz_close(nullptr) == NMZ_OK);
    CHECK(nmz_replayable_plan_destroy(nullptr) == NMZ_OK);
    CHECK(nmz_random_plan_destroy(nullptr) == NMZ_OK);
    CHECK(nmz_ed_plan_destroy(nullptr) == NMZ_OK);
    CHECK(std::strlen(nmz_last_error()) > 0);
}

// ProcSetEvent decisions on the host at the limits (512 processes, prioritized 256: the marked-slot set and the
// attribute rows are written to their last element) and their argument checks
static void procset_cases() {
    nmz_random_params rp;
    nmz_procset_params pp;
    CHECK(nmz_random_params_resolve(30000000, 100000000, 0.1, &rp) == NMZ_OK);
    CHECK(nmz_procset_params_resolve(nullptr, 1, 3, 0.1, &pp) == NMZ_OK && pp.policy == NMZ_PROC_MILD);
    CHECK(nmz_procset_params_resolve("", 0, 3, 0.1, &pp) == NMZ_OK && pp.policy == NMZ_PROC_MILD && !pp.use_batch);
    CHECK(nmz_procset_params_resolve("nope", 1, 3, 0.1, &pp) == NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "bad procPolicy nope") != nullptr);
    CHECK(nmz_procset_params_resolve("dirichlet", 1, 3, 1.5, &pp) == NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "bad procPolicyParam.resetProbability 1.500000") != nullptr);
    CHECK(nmz_procset_params_resolve("dirichlet", 1, 3, std::nan(""), &pp) == NMZ_EINVAL);
    CHECK(nmz_procset_params_resolve("extreme", 1, 257, 0.1, &pp) == NMZ_EINVAL);
    CHECK(nmz_procset_params_resolve("mild", 1, 3, 0.1, nullptr) == NMZ_EINVAL);
    const uint64_t eh[4] = {1, 0x9E3779B97F4A7C15ull, ~0ull, 12345};
    const uint8_t ec[4] = {0, 1, 0, 1};
    uint32_t n[4] = {512, 1, 410, 512};
    std::vector<nmz_proc_attr> at(512 + 1 + 410 + 512);
    int64_t d[4];
    const char *names[3] = {"mild", "extreme", "dirichlet"};
    for (const char *name : names) {
        CHECK(nmz_procset_params_resolve(name, 1, 256, 0.999, &pp) == NMZ_OK);
        for (uint64_t seed = 0; seed < 50; ++seed)
            CHECK(nmz_procset_decide_host(seed, eh, ec, n, 4, &rp, &pp, d, at.data()) == NMZ_OK);
        CHECK(d[0] >= 30000000 && d[0] < 100000000 && d[1] >= 24000000 && d[1] < 80000000);
    }
    CHECK(nmz_procset_decide_host(1, eh, ec, n, 0, &rp, &pp, nullptr, nullptr) == NMZ_OK);
    n[1] = 0;  // dirichlet: an event without a process
    CHECK(nmz_procset_decide_host(1, eh, ec, n, 4, &rp, &pp, d, at.data()) == NMZ_EINVAL);
    n[1] = 513;
    CHECK(nmz_procset_decide_host(1, eh, ec, n, 4, &rp, &pp, d, at.data()) == NMZ_EINVAL);
    n[1] = 1;
    const uint8_t bad[4] = {0, NMZ_EV_FAULTABLE, 0, 0};
    CHECK(nmz_procset_decide_host(1, eh, bad, n, 4, &rp, &pp, d, at.data()) == NMZ_EINVAL);
    CHECK(nmz_procset_decide_host(1, eh, ec, n, 4, &rp, nullptr, d, at.data()) == NMZ_EINVAL);
    CHECK(nmz_procset_decide_host(1, eh, ec, n, 4, nullptr, &pp, d, at.data()) == NMZ_EINVAL);
    CHECK(nmz_procset_decide_host(1, nullptr, ec, n, 4, &rp, &pp, d, at.data()) == NMZ_EINVAL);
    CHECK(nmz_procset_decide(nullptr, 1, eh, ec, n, 4, &rp, &pp, d, at.data()) == NMZ_EINVAL);
    CHECK(nmz_procset_sweep(nullptr, 0, 1, eh, ec, n, nullptr, 4, &rp, &pp, nullptr, nullptr, nullptr, 0, 0, 1,
                            nullptr) == NMZ_EINVAL);
}

// nmz_replayable_order_host (replayablepolicy.go:100-126): a known answer, every limit, optional outputs
static void order_cases() {
    std::vector<uint32_t> off(17, 0);
    std::string bytes;
    std::vector<int64_t> arrival(16);
    for (int i = 0; i < 16; ++i) {
        bytes += "hint-entity-" + std::to_string(i % 4) + "-" + std::to_string(i);
        off[i + 1] = (uint32_t)bytes.size();
        arrival[i] = (int64_t)i * 5000000;
    }
    const uint8_t *hb = reinterpret_cast<const uint8_t *>(bytes.data());
    const nmz_order_constraint cons[5] = {{5, 0, 1000000}, {9, 2, 1000000}, {4, 3, 1}, {12, 7, 10000000}, {14, 1, 1}};
    const uint8_t seed[4] = {'1', '0', '2', '9'};
    nmz_order_stats st;
    int64_t slack[64];
    CHECK(nmz_replayable_order_host(seed, 4, off.data(), hb, 16, 100000000, arrival.data(), cons, 5, &st, slack) ==
          NMZ_OK);
    CHECK(st.n_satisfied == 5 && st.sat_mask == 31 && st.min_slack_ns == 3735120 && st.argmin_constraint == 4);
    CHECK(slack[4] == 3735120);
    CHECK(nmz_replayable_order_host(nullptr, 0, off.data(), hb, 16, 0, arrival.data(), cons, 5, &st, nullptr) == NMZ_OK);
    CHECK(st.n_satisfied == 0 && st.min_slack_ns == -65000001 && st.argmin_constraint == 4);
    CHECK(nmz_replayable_order_host(seed, 4, off.data(), hb, 16, (int64_t)1 << 61, arrival.data(), cons, 5, nullptr,
                                    nullptr) == NMZ_OK);
    std::vector<nmz_order_constraint> many(65, cons[0]);
    CHECK(nmz_replayable_order_host(seed, 4, off.data(), hb, 16, 1, arrival.data(), many.data(), 64, &st, slack) ==
          NMZ_OK);
    CHECK(st.sat_mask == 0 && st.argmin_constraint == 0 && slack[63] == -26000000);
    CHECK(nmz_replayable_order_host(seed, 4, off.data(), hb, 16, 1, arrival.data(), many.data(), 65, &st, slack) ==
          NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "n_constraints") != nullptr);
    CHECK(nmz_replayable_order_host(seed, 4, off.data(), hb, 16, 1, arrival.data(), cons, 0, &st, slack) == NMZ_EINVAL);
    CHECK(nmz_replayable_order_host(seed, 4, off.data(), hb, 16, 1, arrival.data(), nullptr, 1, &st, slack) ==
          NMZ_EINVAL);
    nmz_order_constraint bad = {3, 3, 1};
    CHECK(nmz_replayable_order_host(seed, 4, off.data(), hb, 16, 1, arrival.data(), &bad, 1, &st, slack) == NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "before == after") != nullptr);
    bad = {16, 3, 1};
    CHECK(nmz_replayable_order_host(seed, 4, off.data(), hb, 16, 1, arrival.data(), &bad, 1, &st, slack) == NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "out of range") != nullptr);
    bad = {1, 3, 0};
    CHECK(nmz_replayable_order_host(seed, 4, off.data(), hb, 16, 1, arrival.data(), &bad, 1, &st, slack) == NMZ_EINVAL);
    bad = {1, 3, ((int64_t)1 << 61) + 1};
    CHECK(nmz_replayable_order_host(seed, 4, off.data(), hb, 16, 1, arrival.data(), &bad, 1, &st, slack) == NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "margin_ns") != nullptr);
    CHECK(nmz_replayable_order_host(seed, 4, off.data(), hb, 16, -1, arrival.data(), cons, 5, &st, slack) == NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "max_interval_ns") != nullptr);
    arrival[7] = -1;
    CHECK(nmz_replayable_order_host(seed, 4, off.data(), hb, 16, 1, arrival.data(), cons, 5, &st, slack) == NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "arrival_ns[7]") != nullptr);
    arrival[7] = 35000000;
    CHECK(nmz_replayable_order_host(nullptr, 4, off.data(), hb, 16, 1, arrival.data(), cons, 5, &st, slack) ==
          NMZ_EINVAL);
    // the device entry points reject a NULL context or plan before any device work
    nmz_replayable_order_plan *plan = nullptr;
    nmz_topk_entry tk[2];
    CHECK(nmz_replayable_order_plan_create(nullptr, off.data(), hb, 16, 1, arrival.data(), cons, 5, 10, &plan) ==
          NMZ_EINVAL);
    CHECK(nmz_replayable_order_plan_destroy(nullptr) == NMZ_OK);
    CHECK(nmz_replayable_order_sweep_decimal_dev(nullptr, 0, 1, 1, nullptr, tk, nullptr) == NMZ_EINVAL);
    CHECK(nmz_replayable_order_sweep_dev(nullptr, nullptr, nullptr, 0, 0, 1, nullptr, tk, nullptr) == NMZ_EINVAL);
    CHECK(nmz_replayable_order_sweep(nullptr, off.data(), hb, 1, off.data(), hb, 16, 1, arrival.data(), cons, 5, 1,
                                     nullptr, tk) == NMZ_EINVAL);
    CHECK(nmz_replayable_order_sweep_decimal(nullptr, 0, 1, off.data(), hb, 16, 1, arrival.data(), cons, 5, 1, nullptr,
                                             tk) == NMZ_EINVAL);
}

// nmz_replayable_delivery_host (replayablepolicy.go:100-126, visualize.go:51-136): orders, ties, skipped events,
// the limits (4,096 events, entity 16383), optional outputs
static void delivery_cases() {
    const uint32_t E = NMZ_DELIVERY_MAX_EVENTS;
    std::vector<uint32_t> off(E + 1, 0), ent(E), order(E);
    std::string bytes;
    std::vector<int64_t> arrival(E), rel(E);
    std::vector<uint64_t> sym(E);
    for (uint32_t i = 0; i < E; ++i) {
        bytes += "h" + std::to_string(i % 1000);
        off[i + 1] = (uint32_t)bytes.size();
        arrival[i] = (int64_t)(i / 2) * 1000;
        sym[i] = 0x9E3779B97F4A7C15ull * i;
        ent[i] = i % 7 == 0 ? NMZ_NONE : (i % 5 == 0 ? 16383u : i % 3);
    }
    const uint8_t *hb = reinterpret_cast<const uint8_t *>(bytes.data());
    const uint8_t seed[2] = {'4', '2'};
    nmz_delivery_stats st, st2;
    CHECK(nmz_replayable_delivery_host(seed, 2, off.data(), hb, E, 100000000, arrival.data(), sym.data(), nullptr, &st,
                                       order.data(), rel.data()) == NMZ_OK);
    CHECK(st.n_counted == E && st.min_gap_ns >= 0 && st.gap_event < E);
    for (uint32_t i = 1; i < E; ++i)
        CHECK(rel[order[i - 1]] < rel[order[i]] || (rel[order[i - 1]] == rel[order[i]] && order[i - 1] < order[i]));
    CHECK(nmz_replayable_delivery_host(seed, 2, off.data(), hb, E, (int64_t)1 << 50, arrival.data(), sym.data(),
                                       ent.data(), &st2, order.data(), nullptr) == NMZ_OK);
    CHECK(st2.n_counted == E - (E + 6) / 7 && order[st2.n_counted] == NMZ_NONE && order[E - 1] == NMZ_NONE);
    CHECK(nmz_replayable_delivery_host(nullptr, 0, off.data(), hb, 4, 0, arrival.data(), sym.data(), nullptr, &st,
                                       order.data(), nullptr) == NMZ_OK);
    CHECK(st.n_counted == 4 && st.min_gap_ns == 0 && st.gap_event == 1 && order[0] == 0 && order[3] == 3);
    CHECK(nmz_replayable_delivery_host(seed, 2, off.data(), hb, 1, 5, arrival.data(), sym.data(), nullptr, &st, nullptr,
                                       nullptr) == NMZ_OK);
    CHECK(st.n_counted == 1 && st.min_gap_ns == INT64_MAX && st.gap_event == NMZ_NONE);
    CHECK(nmz_replayable_delivery_host(seed, 2, off.data(), hb, 8, 5, arrival.data(), sym.data(), nullptr, nullptr,
                                       nullptr, nullptr) == NMZ_OK);
    CHECK(nmz_replayable_delivery_host(seed, 2, off.data(), hb, 0, 5, arrival.data(), sym.data(), nullptr, &st, nullptr,
                                       nullptr) == NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "n_events") != nullptr);
    CHECK(nmz_replayable_delivery_host(seed, 2, off.data(), hb, 8, ((int64_t)1 << 50) + 1, arrival.data(), sym.data(),
                                       nullptr, &st, nullptr, nullptr) == NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "max_interval_ns") != nullptr);
    ent[3] = 16384;
    CHECK(nmz_replayable_delivery_host(seed, 2, off.data(), hb, 8, 5, arrival.data(), sym.data(), ent.data(), &st,
                                       nullptr, nullptr) == NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "entity[3]") != nullptr);
    arrival[2] = ((int64_t)1 << 50) + 1;
    CHECK(nmz_replayable_delivery_host(seed, 2, off.data(), hb, 8, 5, arrival.data(), sym.data(), nullptr, &st, nullptr,
                                       nullptr) == NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "arrival_ns[2]") != nullptr);
    CHECK(nmz_replayable_delivery_host(nullptr, 2, off.data(), hb, 8, 5, arrival.data(), sym.data(), nullptr, &st,
                                       nullptr, nullptr) == NMZ_EINVAL);
    // the device entry points reject a NULL context or plan before any device work
    nmz_replayable_delivery_plan *plan = nullptr;
    uint32_t u[2];
    uint64_t sig[2];
    CHECK(nmz_replayable_delivery_plan_create(nullptr, off.data(), hb, 8, 5, arrival.data(), sym.data(), nullptr, 10,
                                              &plan) == NMZ_EINVAL);
    CHECK(nmz_replayable_delivery_plan_destroy(nullptr) == NMZ_OK);
    CHECK(nmz_replayable_delivery_sweep_decimal_dev(nullptr, 0, 1, &st, nullptr) == NMZ_EINVAL);
    CHECK(nmz_replayable_delivery_sweep_dev(nullptr, nullptr, nullptr, 0, &st, nullptr) == NMZ_EINVAL);
    CHECK(nmz_delivery_classes_dev(nullptr, &st, 1, u, u, u, nullptr) == NMZ_EINVAL);
    CHECK(nmz_sig_classes_dev(nullptr, sig, 1, u, nullptr) == NMZ_EINVAL);
    CHECK(nmz_replayable_delivery_sweep(nullptr, off.data(), hb, 1, off.data(), hb, 8, 5, arrival.data(), sym.data(),
                                        nullptr, &st, u, u, u) == NMZ_EINVAL);
    CHECK(nmz_replayable_delivery_sweep_decimal(nullptr, 0, 1, off.data(), hb, 8, 5, arrival.data(), sym.data(),
                                                nullptr, &st, u, u, u) == NMZ_EINVAL);
}

// the run match's host form and the limits of its host-pointer forms (all refused before a context is needed)
static void match_cases() {
    const uint64_t sym[5] = {5, 7, 5, 9, 5};
    const int64_t arrival[5] = {10, 0, 3, 1, 3};
    const uint64_t run[6] = {5, 5, 7, 8, 5, 5};
    uint32_t pos[5];
    CHECK(nmz_match_run_host(sym, arrival, 5, run, 6, pos) == NMZ_OK);
    CHECK(pos[0] == 4 && pos[1] == 2 && pos[2] == 0 && pos[3] == NMZ_NONE && pos[4] == 1);
    CHECK(nmz_match_run_host(sym, arrival, 5, nullptr, 0, pos) == NMZ_OK && pos[0] == NMZ_NONE && pos[4] == NMZ_NONE);
    // a full-size universe of one symbol, over-filled: every position once
    std::vector<uint64_t> one(4096, 42), many(5000, 42);
    std::vector<int64_t> arr(4096);
    std::vector<uint32_t> p(4096);
    for (int i = 0; i < 4096; ++i) arr[i] = (i * 7) % 64;
    CHECK(nmz_match_run_host(one.data(), arr.data(), 4096, many.data(), many.size(), p.data()) == NMZ_OK);
    std::vector<char> seen(4096, 0);
    for (uint32_t v : p) {
        CHECK(v < 4096 && !seen[v]);
        if (v < 4096) seen[v] = 1;
    }
    CHECK(nmz_match_run_host(sym, arrival, 0, run, 6, pos) == NMZ_EINVAL);
    CHECK(nmz_match_run_host(sym, arrival, 5, run, 0xFFFFFFFFull, pos) == NMZ_EINVAL);
    CHECK(nmz_match_run_host(sym, arrival, 5, run, 6, nullptr) == NMZ_EINVAL);
    const uint64_t off[3] = {0, 2, 6}, bad0[3] = {1, 2, 6}, dec[3] = {0, 4, 2};
    uint32_t rows[10];
    const uint8_t failed[2] = {1, 0};
    nmz_order_pair pairs[4];
    CHECK(nmz_match_runs(nullptr, sym, arrival, 5, off, run, 2, rows) == NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "ctx is NULL"));
    CHECK(nmz_match_runs(nullptr, sym, arrival, 5, bad0, run, 2, rows) == NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "run_off[0]"));
    CHECK(nmz_match_runs(nullptr, sym, arrival, 5, dec, run, 2, rows) == NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "non-decreasing"));
    CHECK(nmz_match_runs(nullptr, sym, arrival, 5, off, run, 1ull << 63, rows) == NMZ_EINVAL);
    CHECK(nmz_match_runs(nullptr, sym, arrival, 5, nullptr, nullptr, 0, nullptr) == NMZ_OK);
    CHECK(nmz_order_contrast_runs(nullptr, sym, arrival, 5, off, run, failed, 2, 4, nullptr, pairs, nullptr) ==
          NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "ctx is NULL"));
    CHECK(nmz_order_contrast_runs(nullptr, sym, arrival, 5, dec, run, failed, 2, 4, nullptr, pairs, nullptr) ==
          NMZ_EINVAL);
    nmz_match_plan *plan = nullptr;
    CHECK(nmz_match_plan_create(nullptr, sym, arrival, 5, &plan) == NMZ_EINVAL && plan == nullptr);
    CHECK(nmz_match_plan_destroy(nullptr) == NMZ_OK);
    CHECK(nmz_match_plan_info(nullptr, nullptr, nullptr) == NMZ_EINVAL);
    CHECK(nmz_match_runs_dev(nullptr, off, run, 2, rows, nullptr) == NMZ_EINVAL);
}

// the edit script's host form: the known answers of DESIGN.md section 2 ("Edit scripts"), empty traces, band 0, 64
// and 65, every refusal, and the device forms' NULL plan and context
static std::vector<uint64_t> syms(const char *s) {
    std::vector<uint64_t> v;
    for (; *s; ++s) v.push_back(0x9E3779B97F4A7C15ull * (uint64_t)(unsigned char)*s + 5);
    return v;
}

static bool script_is(const char *a, const char *b, uint32_t band, uint32_t want_dist,
                      std::vector<nmz_edit_op> want) {
    const std::vector<uint64_t> va = syms(a), vb = syms(b);
    std::vector<nmz_edit_op> ops(band ? band : 1, nmz_edit_op{7, 7, 7});
    uint32_t dist = 99;
    nmz_edit_op *po = band ? ops.data() : nullptr;
    if (nmz_ed_align_host(va.data(), va.size(), vb.data(), vb.size(), band, &dist, po) != NMZ_OK) return false;
    if (dist != want_dist) return false;
    want.resize(band, nmz_edit_op{NMZ_NONE, NMZ_NONE, NMZ_NONE});
    for (uint32_t s = 0; s < band; ++s)
        if (ops[s].a_pos != want[s].a_pos || ops[s].b_pos != want[s].b_pos || ops[s].kind != want[s].kind) return false;
    return true;
}

static void align_cases() {
    const uint32_t S = NMZ_EDIT_SUB, D = NMZ_EDIT_DEL, I = NMZ_EDIT_INS;
    CHECK(script_is("kitten", "sitting", 3, 3, {{0, 0, S}, {4, 4, S}, {6, 6, I}}));
    CHECK(script_is("kitten", "sitting", 2, 3, {}));
    CHECK(script_is("abc", "", 3, 3, {{0, 0, D}, {1, 0, D}, {2, 0, D}}));
    CHECK(script_is("", "ab", 2, 2, {{0, 0, I}, {0, 1, I}}));
    CHECK(script_is("ab", "ba", 2, 2, {{0, 0, S}, {1, 1, S}}));
    CHECK(script_is("aab", "ab", 1, 1, {{0, 0, D}}));
    CHECK(script_is("ab", "aab", 1, 1, {{0, 0, I}}));
    CHECK(script_is("abcde", "bcdex", 2, 2, {{0, 0, D}, {5, 4, I}}));
    CHECK(script_is("abab", "baba", 2, 2, {{0, 0, I}, {3, 4, D}}));
    CHECK(script_is("aaaa", "aa", 2, 2, {{0, 0, D}, {1, 0, D}}));
    CHECK(script_is("", "", 4, 0, {}));
    CHECK(script_is("", "", 0, 0, {}));
    CHECK(script_is("abc", "abc", 0, 0, {}));
    CHECK(script_is("abc", "abd", 0, 1, {}));
    CHECK(script_is("abc", "ab", 0, 1, {}));
    // band 64: 64 deletions at the band's edge, then one more than the band holds; band 65 is refused
    std::vector<uint64_t> a(200), b;
    for (size_t i = 0; i < a.size(); ++i) a[i] = 1000 + i;
    b.assign(a.begin() + 64, a.end());
    std::vector<nmz_edit_op> ops(65);
    uint32_t dist = 0;
    CHECK(nmz_ed_align_host(a.data(), a.size(), b.data(), b.size(), 64, &dist, ops.data()) == NMZ_OK && dist == 64);
    for (uint32_t s = 0; s < 64; ++s) CHECK(ops[s].a_pos == s && ops[s].b_pos == 0 && ops[s].kind == D);
    CHECK(nmz_ed_align_host(b.data(), b.size(), a.data(), a.size(), 64, &dist, ops.data()) == NMZ_OK && dist == 64);
    for (uint32_t s = 0; s < 64; ++s) CHECK(ops[s].a_pos == 0 && ops[s].b_pos == s && ops[s].kind == I);
    CHECK(nmz_ed_align_host(a.data(), a.size(), b.data() + 1, b.size() - 1, 64, &dist, ops.data()) == NMZ_OK);
    CHECK(dist == 65 && ops[0].kind == NMZ_NONE && ops[63].a_pos == NMZ_NONE);
    CHECK(nmz_ed_align_host(a.data(), a.size(), b.data(), b.size(), 65, &dist, ops.data()) == NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "NMZ_ALIGN_MAX_BAND") != nullptr);
    CHECK(nmz_ed_align_host(a.data(), 0xFFFFFFFFull, b.data(), 3, 4, &dist, ops.data()) == NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "at most 2^32 - 2") != nullptr);
    CHECK(nmz_ed_align_host(a.data(), 3, b.data(), 0xFFFFFFFFull, 4, &dist, ops.data()) == NMZ_EINVAL);
    CHECK(nmz_ed_align_host(nullptr, 3, b.data(), 3, 4, &dist, ops.data()) == NMZ_EINVAL);
    CHECK(nmz_ed_align_host(a.data(), 3, nullptr, 3, 4, &dist, ops.data()) == NMZ_EINVAL);
    CHECK(nmz_ed_align_host(a.data(), 3, b.data(), 3, 4, nullptr, ops.data()) == NMZ_EINVAL);
    CHECK(nmz_ed_align_host(a.data(), 3, b.data(), 3, 4, &dist, nullptr) == NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "ops is NULL") != nullptr);
    CHECK(nmz_ed_align_host(nullptr, 0, nullptr, 0, 0, &dist, nullptr) == NMZ_OK && dist == 0);
    // the host-pointer form: every refusal comes before the context is looked at
    const uint64_t off[4] = {0, 3, 3, 8}, dec[4] = {0, 5, 3, 8}, big[3] = {0, 0xFFFFFFFFull, 0x100000000ull};
    const uint32_t pairs[4] = {0, 2, 1, 1}, bad[2] = {0, 3};
    uint32_t d2[2];
    CHECK(nmz_ed_align_pairs(nullptr, off, a.data(), 3, pairs, 2, 8, d2, ops.data()) == NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "ctx is NULL") != nullptr);
    CHECK(nmz_ed_align_pairs(nullptr, off, a.data(), 3, pairs, 2, 65, d2, ops.data()) == NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "wider bands") != nullptr);
    CHECK(nmz_ed_align_pairs(nullptr, off, a.data(), 3, bad, 1, 8, d2, ops.data()) == NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "pair index out of range") != nullptr);
    CHECK(nmz_ed_align_pairs(nullptr, dec, a.data(), 3, pairs, 2, 8, d2, ops.data()) == NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "non-decreasing") != nullptr);
    CHECK(nmz_ed_align_pairs(nullptr, big, a.data(), 2, pairs + 2, 1, 8, d2, ops.data()) == NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "trace 0 has 4294967295 elements") != nullptr);
    CHECK(nmz_ed_align_pairs(nullptr, off, a.data(), 3, pairs, 2, 8, nullptr, ops.data()) == NMZ_EINVAL);
    CHECK(nmz_ed_align_pairs(nullptr, off, a.data(), 3, pairs, 2, 8, d2, nullptr) == NMZ_EINVAL);
    CHECK(nmz_ed_align_pairs(nullptr, nullptr, nullptr, 0, nullptr, 0, 8, nullptr, nullptr) == NMZ_OK);
    CHECK(nmz_ed_align_pairs(nullptr, nullptr, nullptr, 0, nullptr, 0, 65, nullptr, nullptr) == NMZ_EINVAL);
    // the plan and the device form
    nmz_ed_align_plan *plan = reinterpret_cast<nmz_ed_align_plan *>(0x1);
    CHECK(nmz_ed_align_plan_create(nullptr, 8, 100, &plan) == NMZ_EINVAL && plan == nullptr);
    CHECK(std::strstr(nmz_last_error(), "ctx is NULL") != nullptr);
    CHECK(nmz_ed_align_plan_create(nullptr, 65, 100, &plan) == NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "NMZ_ALIGN_MAX_BAND") != nullptr);
    CHECK(nmz_ed_align_plan_create(nullptr, 64, 1ull << 30, &plan) == NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "max_len 1073741824") != nullptr && std::strstr(nmz_last_error(), "budget"));
    CHECK(nmz_ed_align_plan_create(nullptr, 8, 0xFFFFFFFFull, &plan) == NMZ_EINVAL);
    CHECK(nmz_ed_align_plan_create(nullptr, 8, 100, nullptr) == NMZ_EINVAL);
    CHECK(nmz_ed_align_plan_destroy(nullptr) == NMZ_OK);
    CHECK(nmz_ed_align_plan_info(nullptr, nullptr, nullptr) == NMZ_EINVAL);
    CHECK(nmz_ed_align_pairs_dev(nullptr, off, a.data(), pairs, 2, d2, ops.data(), nullptr) == NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "plan is NULL") != nullptr);
}

// the move profile's host forms: the known answers of DESIGN.md section 2 ("Move profiles") through
// nmz_ed_align_host's scripts, a full band whose last slot has a partner 32 slots away, a table without one symbol,
// an empty table, no pairs, and the refusals (the device forms' come before the context is looked at)
static void moves_cases() {
    const uint32_t D = NMZ_EDIT_DEL, I = NMZ_EDIT_INS, NONE = NMZ_NONE;
    // abab -> baba, w = 2: INS(0, 0) DEL(3, 4) are partners, b moves earlier over a span of 4
    const std::vector<uint64_t> ab = syms("abab"), ba = syms("baba");
    std::vector<uint64_t> sym(ab);
    sym.insert(sym.end(), ba.begin(), ba.end());
    const uint64_t off[3] = {0, 4, 8};
    const uint32_t pairs[4] = {0, 1, 1, 1};
    uint32_t dist[2] = {9, 9};
    std::vector<nmz_edit_op> ops(4);
    for (int p = 0; p < 2; ++p)
        CHECK(nmz_ed_align_host(sym.data() + off[pairs[2 * p]], 4, sym.data() + off[pairs[2 * p + 1]], 4, 2, &dist[p],
                                ops.data() + 2 * p) == NMZ_OK);
    CHECK(dist[0] == 2 && dist[1] == 0 && ops[0].kind == I && ops[1].kind == D);
    uint32_t pr2[2] = {7, 7};
    CHECK(nmz_script_moves_host(ab.data(), 4, ba.data(), 4, ops.data(), 2, pr2) == NMZ_OK && pr2[0] == 1 && pr2[1] == 0);
    uint64_t usym[2] = {syms("a")[0], syms("b")[0]};
    if (usym[0] > usym[1]) std::swap(usym[0], usym[1]);
    const int ib = usym[0] == syms("b")[0] ? 0 : 1;
    nmz_move_counts counts[2];
    nmz_move_info info;
    uint32_t partner[4] = {7, 7, 7, 7};
    CHECK(nmz_move_profile_host(off, sym.data(), 2, pairs, 2, 2, dist, ops.data(), usym, 2, partner, counts, &info) ==
          NMZ_OK);
    CHECK(partner[0] == 1 && partner[1] == 0 && partner[2] == NONE && partner[3] == NONE);
    CHECK(info.n_scripts == 2 && info.n_beyond == 0 && info.n_ops == 2 && info.n_unknown == 0);
    CHECK(counts[ib].earlier == 1 && counts[ib].span_earlier == 4 && counts[ib].n_pairs == 1 && counts[ib].later == 0);
    CHECK(counts[1 - ib].n_pairs == 0 && counts[1 - ib].earlier == 0 && counts[ib].reserved == 0);
    // the table without b, then no table: the names are unknown, the partners stay
    const uint64_t only_a = syms("a")[0];
    CHECK(nmz_move_profile_host(off, sym.data(), 2, pairs, 2, 2, dist, ops.data(), &only_a, 1, partner, counts, &info) ==
          NMZ_OK);
    CHECK(info.n_unknown == 2 && counts[0].n_pairs == 0 && partner[0] == 1 && partner[1] == 0);
    CHECK(nmz_move_profile_host(off, sym.data(), 2, pairs, 2, 2, dist, ops.data(), nullptr, 0, nullptr, nullptr, &info) ==
          NMZ_OK);
    CHECK(info.n_unknown == 2 && info.n_ops == 2);
    // X^32 + B -> B + X^32, w = 64: 32 DELs, then 32 INSs, partner[s] = s + 32, all later
    std::vector<uint64_t> a, b;
    for (int r = 0; r < 32; ++r) a.push_back(5000);
    for (int t = 0; t < 66; ++t) a.push_back(100 + t), b.push_back(100 + t);
    for (int r = 0; r < 32; ++r) b.push_back(5000);
    std::vector<nmz_edit_op> o64(64);
    std::vector<uint32_t> p64(64, 7);
    uint32_t d64 = 0;
    CHECK(nmz_ed_align_host(a.data(), a.size(), b.data(), b.size(), 64, &d64, o64.data()) == NMZ_OK && d64 == 64);
    CHECK(nmz_script_moves_host(a.data(), a.size(), b.data(), b.size(), o64.data(), 64, p64.data()) == NMZ_OK);
    for (uint32_t s = 0; s < 32; ++s) CHECK(o64[s].kind == D && p64[s] == s + 32 && p64[s + 32] == s);
    std::vector<uint64_t> both(a);
    both.insert(both.end(), b.begin(), b.end());
    const uint64_t off2[3] = {0, a.size(), a.size() + b.size()}, x = 5000;
    const uint32_t fwd[2] = {0, 1};
    nmz_move_counts cx;
    CHECK(nmz_move_profile_host(off2, both.data(), 2, fwd, 1, 64, &d64, o64.data(), &x, 1, p64.data(), &cx, &info) ==
          NMZ_OK);
    CHECK(cx.later == 32 && cx.earlier == 0 && cx.n_pairs == 1 && cx.span_later == 32 * 66 + 496 && p64[63] == 31);
    // no pairs: zeros, from every form, without a device
    cx.later = 7;
    info.n_ops = 7;
    CHECK(nmz_move_profile_host(nullptr, nullptr, 0, nullptr, 0, 8, nullptr, nullptr, &x, 1, nullptr, &cx, &info) == NMZ_OK);
    CHECK(cx.later == 0 && info.n_ops == 0);
    cx.later = 7;
    CHECK(nmz_move_profile(nullptr, nullptr, nullptr, 0, nullptr, 0, 8, nullptr, nullptr, &x, 1, nullptr, &cx, &info) ==
          NMZ_OK && cx.later == 0);
    cx.later = 7;
    CHECK(nmz_ed_diff_profile(nullptr, nullptr, nullptr, 0, nullptr, 0, 8, &x, 1, nullptr, &cx, &info) == NMZ_OK &&
          cx.later == 0);
    // refusals
    CHECK(nmz_move_profile_host(off, sym.data(), 2, pairs, 2, 65, dist, ops.data(), usym, 2, partner, counts, &info) ==
          NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "wider bands") != nullptr);
    const uint64_t same[2] = {usym[0], usym[0]};
    CHECK(nmz_move_profile_host(off, sym.data(), 2, pairs, 2, 2, dist, ops.data(), same, 2, partner, counts, &info) ==
          NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "strictly increasing") != nullptr);
    CHECK(nmz_move_profile_host(off, sym.data(), 2, pairs, 1ull << 31, 2, dist, ops.data(), usym, 2, partner, counts,
                                &info) == NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "below 2^32") != nullptr);
    std::vector<nmz_edit_op> bad(ops);
    bad[1].a_pos = 4;
    CHECK(nmz_move_profile_host(off, sym.data(), 2, pairs, 2, 2, dist, bad.data(), usym, 2, partner, counts, &info) ==
          NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "a_pos 4 is outside") != nullptr);
    bad[1] = nmz_edit_op{3, 4, 7};
    CHECK(nmz_script_moves_host(ab.data(), 4, ba.data(), 4, bad.data(), 2, pr2) == NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "op kind 7") != nullptr);
    CHECK(nmz_move_profile(nullptr, off, sym.data(), 2, pairs, 2, 2, dist, ops.data(), usym, 2, partner, counts, &info) ==
          NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "ctx is NULL") != nullptr);
    CHECK(nmz_ed_diff_profile(nullptr, off, sym.data(), 2, pairs, 2, 2, usym, 2, nullptr, counts, &info) == NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "ctx is NULL") != nullptr);
    CHECK(nmz_move_profile_dev(nullptr, off, sym.data(), pairs, 2, 2, dist, ops.data(), usym, 2, partner, counts, &info, 0,
                               nullptr) == NMZ_EINVAL);
    // the wide forms: the same rotation through band 70 (6 sentinel slots behind the 64 ops), then the refusals
    std::vector<nmz_edit_op> o70(70);
    std::vector<uint32_t> p70(70, 7);
    uint32_t d70 = 0;
    CHECK(nmz_ed_align_wide_host(a.data(), a.size(), b.data(), b.size(), 70, &d70, o70.data()) == NMZ_OK && d70 == 64);
    CHECK(nmz_move_profile_wide_host(off2, both.data(), 2, fwd, 1, 70, &d70, o70.data(), &x, 1, p70.data(), &cx, &info) ==
          NMZ_OK);
    CHECK(cx.later == 32 && cx.n_pairs == 1 && cx.span_later == 32 * 66 + 496 && p70[63] == 31 && p70[69] == NONE);
    CHECK(info.n_scripts == 1 && info.n_ops == 64);
    CHECK(nmz_move_profile_wide_host(off2, both.data(), 2, fwd, 1, 1025, &d70, o70.data(), &x, 1, p70.data(), &cx,
                                     &info) == NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "NMZ_ALIGN_WIDE_MAX_BAND") != nullptr);
    o70[40].kind = 7;
    CHECK(nmz_move_profile_wide_host(off2, both.data(), 2, fwd, 1, 70, &d70, o70.data(), &x, 1, p70.data(), &cx, &info) ==
          NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "pair 0, slot 40") != nullptr);
    CHECK(nmz_move_profile_wide(nullptr, nullptr, nullptr, 0, nullptr, 0, 512, nullptr, nullptr, &x, 1, nullptr, &cx,
                                &info) == NMZ_OK && cx.later == 0);
    CHECK(nmz_ed_diff_profile_wide(nullptr, off2, both.data(), 2, fwd, 1, 512, &x, 1, nullptr, &cx, &info) == NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "ctx is NULL") != nullptr);
    CHECK(nmz_move_profile_wide_dev(nullptr, off2, both.data(), fwd, 1, 512, &d70, o70.data(), &x, 1, nullptr, &cx, &info,
                                    0, nullptr) == NMZ_EINVAL);
    // per entity: everything in one entity gives the wide form's bytes; X and the block in two entities gives an
    // empty script; then the refusals, each before the context
    std::vector<uint32_t> e1(std::max(a.size(), b.size()), 0), ea(a.size()), eb(b.size()), eboth;
    for (size_t i = 0; i < a.size(); ++i) ea[i] = a[i] == x ? 0 : 1;
    for (size_t i = 0; i < b.size(); ++i) eb[i] = b[i] == x ? 0 : 1;
    eboth.insert(eboth.end(), ea.begin(), ea.end());
    eboth.insert(eboth.end(), eb.begin(), eb.end());
    std::vector<nmz_edit_op> w70(70), q70(70);
    uint32_t dq = 0;
    CHECK(nmz_ed_align_wide_host(a.data(), a.size(), b.data(), b.size(), 70, &d70, w70.data()) == NMZ_OK && d70 == 64);
    CHECK(nmz_ed_align_po_host(a.data(), e1.data(), a.size(), b.data(), e1.data(), b.size(), 1, 70, &dq, q70.data()) ==
              NMZ_OK && dq == 64 && std::memcmp(w70.data(), q70.data(), 70 * sizeof(nmz_edit_op)) == 0);
    CHECK(nmz_ed_align_po_host(a.data(), ea.data(), a.size(), b.data(), eb.data(), b.size(), 2, 70, &dq, q70.data()) ==
              NMZ_OK && dq == 0 && q70[0].kind == NONE);
    CHECK(nmz_ed_align_po_host(a.data(), ea.data(), a.size(), b.data(), eb.data(), b.size(), 1, 70, &dq, q70.data()) ==
          NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "ids are < n_entities (1) or NMZ_NONE") != nullptr);
    CHECK(nmz_ed_align_po_host(a.data(), ea.data(), a.size(), b.data(), eb.data(), b.size(), 1025, 70, &dq,
                               q70.data()) == NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "NMZ_PO_MAX_ENTITIES") != nullptr);
    CHECK(nmz_ed_align_po_pairs(nullptr, off2, both.data(), eboth.data(), 2, 2, fwd, 1, 70, &dq, q70.data()) ==
          NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "ctx is NULL") != nullptr);
    CHECK(nmz_ed_align_po_pairs(nullptr, off2, both.data(), eboth.data(), 2, 1, fwd, 1, 70, &dq, q70.data()) ==
          NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "has entity id 1") != nullptr);
    CHECK(nmz_ed_diff_profile_po(nullptr, off2, both.data(), eboth.data(), 2, 2, fwd, 1, 512, &x, 1, nullptr, &cx,
                                 &info) == NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "ctx is NULL") != nullptr);
    std::vector<uint64_t> poff(2 * 2 + 1), psym(both.size());
    std::vector<uint32_t> psrc(both.size());
    CHECK(nmz_po_project(nullptr, off2, both.data(), eboth.data(), 2, 2, poff.data(), psym.data(), psrc.data()) ==
          NMZ_EINVAL);
    CHECK(std::strstr(nmz_last_error(), "ctx is NULL") != nullptr);
    nmz_ed_align_po_plan *pp = nullptr;
    CHECK(nmz_ed_align_po_plan_create(nullptr, 70, 2, 100, 0, &pp) == NMZ_EINVAL && pp == nullptr);
    CHECK(std::strstr(nmz_last_error(), "max_pairs is 0") != nullptr);
}

// ScratchLayout (scratch_layout.h) over a host buffer that holds exactly the bytes asked for: under ASan a field
// that reached past the buffer, or a write through a pointer that was never placed, is an error
struct FakeBuf {
    void *ptr = nullptr;
    size_t cap = 0;
    const char *slot = nullptr;
    bool busy = false;
    int ensures = 0;
    int ensure(size_t bytes) {
        ++ensures;
        std::free(ptr);
        ptr = std::malloc(bytes);
        cap = bytes;
        return ptr ? NMZ_OK : NMZ_ENOMEM;
    }
    ~FakeBuf() { std::free(ptr); }
};

template <typename T>
static size_t rounded(size_t count) { return (count * sizeof(T) + 255) & ~size_t(255); }

static void layout_cases() {
    static_assert(sizeof(nmz_proc_attr) == 16 && sizeof(nmz_topk_entry) == 24, "the 16- and 24-byte element types");
    {  // mixed element sizes: offsets, total, and a write of every field's full extent
        uint8_t *a;
        uint16_t *b;
        uint32_t *c;
        uint64_t *d;
        nmz_proc_attr *e;
        nmz_topk_entry *f;
        nmz_move_counts *g;
        const size_t n[7] = {3, 129, 65, 33, 17, 11, 5};
        nmz::ScratchLayout lay;
        lay.add(&a, n[0]).add(&b, n[1]).add(&c, n[2]).add(&d, n[3]).add(&e, n[4]).add(&f, n[5]).add(&g, n[6]);
        const size_t want[7] = {rounded<uint8_t>(n[0]),       rounded<uint16_t>(n[1]),       rounded<uint32_t>(n[2]),
                                rounded<uint64_t>(n[3]),      rounded<nmz_proc_attr>(n[4]),  rounded<nmz_topk_entry>(n[5]),
                                rounded<nmz_move_counts>(n[6])};
        size_t sum = 0;
        for (size_t w : want) sum += w;
        CHECK(lay.bytes() == sum);
        FakeBuf buf;
        CHECK(lay.bind(buf) == NMZ_OK && buf.ensures == 1 && buf.cap == sum);
        char *base = static_cast<char *>(buf.ptr);
        char *at[7] = {(char *)a, (char *)b, (char *)c, (char *)d, (char *)e, (char *)f, (char *)g};
        size_t off = 0;
        for (int i = 0; i < 7; ++i) {
            CHECK(at[i] == base + off && off % 256 == 0);
            CHECK(i == 0 || at[i] > at[i - 1]);
            off += want[i];
        }
        std::memset(a, 1, n[0] * sizeof *a);
        std::memset(b, 2, n[1] * sizeof *b);
        std::memset(c, 3, n[2] * sizeof *c);
        std::memset(d, 4, n[3] * sizeof *d);
        std::memset(e, 5, n[4] * sizeof *e);
        std::memset(f, 6, n[5] * sizeof *f);
        std::memset(g, 7, n[6] * sizeof *g);
        // no field reached into its neighbour: each one's first and last byte still hold its own value
        CHECK(a[0] == 1 && b[0] == 0x0202 && ((char *)c)[n[2] * 4 - 1] == 3 && ((char *)g)[0] == 7);
        CHECK(((char *)f)[n[5] * 24 - 1] == 6 && ((char *)e)[0] == 5 && ((char *)d)[n[3] * 8 - 1] == 4);
    }
    {  // a zero-count field takes no space and has the address of the field after it, or of the buffer's end
        uint64_t *x, *z_mid, *y, *z_end;
        nmz::ScratchLayout lay;
        lay.add(&x, 10).add(&z_mid, 0).add(&y, 40).add(&z_end, 0);
        CHECK(lay.bytes() == rounded<uint64_t>(10) + rounded<uint64_t>(40));
        FakeBuf buf;
        CHECK(lay.bind(buf) == NMZ_OK);
        char *base = static_cast<char *>(buf.ptr);
        CHECK((char *)z_mid == (char *)y && (char *)y == base + 256);
        CHECK((char *)z_end == base + lay.bytes());
        std::memset(x, 0, 10 * 8);
        std::memset(y, 0, 40 * 8);
    }
    {  // one field more than the capacity: an error, no allocation, no pointer written
        uint32_t *p[nmz::ScratchLayout::CAP + 1];
        for (auto &q : p) q = reinterpret_cast<uint32_t *>(0x10);
        nmz::ScratchLayout lay;
        for (auto &q : p) lay.add(&q, 4);
        FakeBuf buf;
        CHECK(lay.bind(buf) == NMZ_EINVAL && buf.ensures == 0 && buf.ptr == nullptr);
        CHECK(std::strstr(nmz_last_error(), "fields") != nullptr);
        CHECK(lay.place(nullptr) == NMZ_EINVAL);
        for (auto &q : p) CHECK(q == reinterpret_cast<uint32_t *>(0x10));
    }
    {  // count * sizeof(T), its rounding, and the running sum must not wrap
        uint64_t *p;
        uint8_t *q, *r;
        FakeBuf buf;
        nmz::ScratchLayout mul, rnd, sum;
        CHECK(mul.add(&p, SIZE_MAX / 4).bind(buf) == NMZ_ENOMEM);
        CHECK(rnd.add(&q, SIZE_MAX - 100).bind(buf) == NMZ_ENOMEM);
        CHECK(sum.add(&q, SIZE_MAX / 2).add(&r, SIZE_MAX / 2 + 512).bind(buf) == NMZ_ENOMEM);
        CHECK(buf.ensures == 0);
    }
    {  // a named slot is marked while a layout is bound to it: a second bind is refused, by name
        FakeBuf buf;
        buf.slot = "SLOT_DRIVER_TEST";
        uint32_t *p, *q;
        {
            nmz::ScratchLayout outer;
            CHECK(outer.add(&p, 8).bind(buf) == NMZ_OK && buf.busy);
            nmz::ScratchLayout inner;
            CHECK(inner.add(&q, 8000).bind(buf) == NMZ_EINVAL && buf.ensures == 1);
            CHECK(std::strstr(nmz_last_error(), "SLOT_DRIVER_TEST") != nullptr);
            std::memset(p, 0, 8 * 4);  // the outer pointer is still good
        }
        CHECK(!buf.busy);
        nmz::ScratchLayout again;
        CHECK(again.add(&q, 8000).bind(buf) == NMZ_OK && buf.ensures == 2);
        std::memset(q, 0, 8000 * 4);
    }
}

static void no_device_cases() {
    nmz_ctx *c = reinterpret_cast<nmz_ctx *>(0x1);
    int rc = nmz_open(0, &c);
    // no GPU in this container: a clean error and a NULL context (on a GPU box this opens device 0)
    if (rc == NMZ_OK) {
        CHECK(c != nullptr);
        nmz_close(c);
    } else {
        CHECK(c == nullptr && std::strlen(nmz_last_error()) > 0);
    }
    CHECK(nmz_open(-1, &c) != NMZ_OK && c == nullptr);
    CHECK(nmz_open(0, nullptr) == NMZ_EINVAL);
    int n = -1;
    rc = nmz_device_count(&n);
    CHECK(rc != NMZ_OK || n >= 0);
    CHECK(nmz_device_count(nullptr) == NMZ_EINVAL);
    CHECK(nmz_abi_version() == NMZ_ABI_VERSION);
}

// every thread's nmz_last_error() reports its own latest failure (thread-local), under concurrency
static void thread_local_errors(int n_threads, int iters) {
    std::vector<std::thread> ts;
    for (int t = 0; t < n_threads; ++t) {
        ts.emplace_back([t, iters] {
            nmz_random_params p;
            for (int i = 0; i < iters; ++i) {
                const bool bad_p = ((i + t) % 3) == 0, bad_range = ((i + t) % 3) == 1;
                const int rc = nmz_random_params_resolve(bad_range ? 100 + t : t, 50 + i % 7, bad_p ? 2.0 : 0.25, &p);
                if (bad_p) {
                    CHECK(rc == NMZ_EINVAL && std::strstr(nmz_last_error(), "faultActionProbability"));
                } else if (bad_range) {
                    CHECK(rc == NMZ_EINVAL && std::strstr(nmz_last_error(), "minDuration"));
                } else {
                    CHECK(rc == NMZ_OK && p.fault_threshold == 250);
                }
                CHECK(nmz_ed_pairs(nullptr, nullptr, nullptr, 0, nullptr, 0, 0, nullptr) == NMZ_EINVAL);
                CHECK(std::strstr(nmz_last_error(), "ctx is NULL"));
            }
        });
    }
    for (auto &th : ts) th.join();
}

int main() {
    params_cases();
    null_ctx_cases();
    procset_cases();
    order_cases();
    delivery_cases();
    match_cases();
    align_cases();
    moves_cases();
    layout_cases();
    no_device_cases();
    thread_local_errors(8, 2000);
    if (g_fail) {
        std::fprintf(stderr, "%d checks failed\n", g_fail.load());
        return 1;
    }
    std::printf("host ABI checks ok\n");
    return 0;
}
