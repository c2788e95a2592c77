// Cross-translation-unit declarations inside libnmz_gpu.so.
#pragma once
#include "nmz_common.h"

namespace nmz {

uint64_t topk_scratch_entries(uint64_t n, uint32_t k);
int topk_merge_lists(hipStream_t st, nmz_topk_entry *a, nmz_topk_entry *b, uint64_t lists, uint32_t k,
                     nmz_topk_entry *d_out);
int topk_select(hipStream_t st, const nmz_sched_stats *d_stats, uint64_t n, uint64_t seed0, uint32_t k,
                nmz_topk_entry *d_scratch, nmz_topk_entry *d_out);

// unique.hip: sorted distinct symbols on the device (hipcub radix sort + unique); *n_uniq on the host
int device_unique_u64(const uint64_t *d_sym, uint64_t total, uint64_t *d_uniq, uint64_t cap, uint64_t *n_uniq,
                      hipStream_t st);
// unique.hip, for delivery.hip: the per-context table of the signature's rank keys (sig_dev.h; RANK_KEYS entries,
// built on first use), and the equality classes of d_sig[2 * N]: first[i] = the smallest j with sig_j == sig_i
// (radix sort with the index as payload; scratch SLOT_CLASSES). The caller holds ctx.
int sig_rank_keys(nmz_ctx *ctx, const ulonglong2 **out);
int classes_launch(nmz_ctx *ctx, const uint64_t *d_sig, uint32_t N, uint32_t *d_first, hipStream_t st);

// match.hip, for contrast.hip (nmz_order_contrast_runs). match_validate: every limit of the host forms, no device.
int match_validate(const uint64_t *sym, const int64_t *arrival, uint32_t E, const uint64_t *run_off,
                   const uint64_t *run_sym, uint64_t n_runs);
// One host-form match on the context's stream; the caller holds ctx and has validated. Builds the universe's plan
// (the call owns it), takes rows, offsets and symbols from the context's pool as call.work, uploads the CSR and
// enqueues the match: *d_pos = the [n_runs][E] rows.
int match_call(nmz_ctx *ctx, HostCall &call, const uint64_t *sym, const int64_t *arrival, uint32_t E,
               const uint64_t *run_off, const uint64_t *run_sym, uint64_t n_runs, uint32_t **d_pos);

// "This plan's scratch serves one stream at a time": the stream the plan's launches were enqueued on last, with an
// event after the latest one. A launch on another stream first waits for that event; destroy waits for it on the host.
// The messages of a failing call name it as the plans' own code did, hence `p`.
struct PlanFence {
    hipStream_t last = nullptr;
    hipEvent_t ev = nullptr;
    int create(const char *what) {  // what: the plan's name in the message
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess) return NMZ_OK;
        ev = nullptr;
        return fail(NMZ_EHIP, std::string(what) + ": hipEventCreate failed");
    }
    int enter(hipStream_t st) {  // before the plan's launches on st
        PlanFence *p = this;  // for the message's text
        if (p->last && p->last != st) NMZ_HIP(hipStreamWaitEvent(st, p->ev, 0));
        return NMZ_OK;
    }
    int leave(hipStream_t st) {  // behind them, whether or not they all went out
        PlanFence *p = this;  // for the message's text
        p->last = st;
        NMZ_HIP(hipEventRecord(p->ev, st));
        return NMZ_OK;
    }
    void destroy() {
        if (!ev) return;
        (void)hipEventSynchronize(ev);
        (void)hipEventDestroy(ev);
        ev = nullptr;
    }
};

// ed_align.hip: the host side that the aligners share, for ed_align_wide.hip (K8w), ed_moves.hip (nmz_move_profile,
// nmz_ed_diff_profile) and ed_po.hip. The kernels' shared device side is ed_align_dev.h.
// align_len: a trace length is 0 .. 2^32 - 2. align_history_fits: one pair's history against ALIGN_BUDGET, the
// history scratch of a plan (all slots together).
constexpr size_t ALIGN_BUDGET = (size_t)256 << 20;
int align_len(const std::string &what, uint64_t len);
int align_history_fits(uint64_t max_len, uint64_t slot_words);
// The one validator body behind align_validate (band_ok = align_band, max_band = NMZ_ALIGN_MAX_BAND) and aw_validate
// (aw_band, NMZ_ALIGN_WIDE_MAX_BAND; ed_plan.h): every limit of the *_pairs host forms, no device; *max_len = the
// longest trace of the pairs.
int align_validate_for(int (*band_ok)(uint32_t), uint32_t max_band, const uint64_t *off, const uint64_t *sym,
                       uint32_t n_traces, const uint32_t *pairs, uint64_t n_pairs, uint32_t band, const uint32_t *dist,
                       const nmz_edit_op *ops, uint64_t *max_len);
// The one host aligner behind nmz_ed_align_host (Cell = uint8_t) and nmz_ed_align_wide_host (uint16_t), behind the
// entry point's band check: a Cell holds band + 1. fn and cells ("cells", "16-bit cells") go into the messages.
template <typename Cell>
int align_host(const char *fn, const char *cells, const uint64_t *a, uint64_t n, const uint64_t *b, uint64_t m,
               uint32_t band, uint32_t *dist, nmz_edit_op *ops);
// ed_align_wide.hip: the host-arrays form behind nmz_ed_align_pairs and nmz_ed_align_wide_pairs, after the entry
// point's validation and shape: a wide plan for the call (which owns a narrow one for a band <= 64), upload, enqueue,
// download.
int align_pairs_call(nmz_ctx *ctx, const uint64_t *off, const uint64_t *sym, uint32_t n_traces, const uint32_t *pairs,
                     uint64_t n_pairs, uint32_t band, uint64_t max_len, uint64_t slot_words, uint32_t *dist,
                     nmz_edit_op *ops);
// align_validate: every limit of nmz_ed_align_pairs. align_shape: the plan's shape for (band, max_len), no device.
// The _locked forms and align_enqueue want the caller to hold the context.
int align_band(uint32_t band);
int align_validate(const uint64_t *off, const uint64_t *sym, uint32_t n_traces, const uint32_t *pairs,
                   uint64_t n_pairs, uint32_t band, const uint32_t *dist, const nmz_edit_op *ops, uint64_t *max_len);
int align_shape(uint32_t band, uint64_t max_len, uint64_t *slot_words);
int align_plan_create_locked(nmz_ctx *ctx, uint32_t band, uint64_t max_len, uint64_t slot_words,
                             nmz_ed_align_plan **out);
void align_plan_destroy_locked(nmz_ed_align_plan *p);
int align_enqueue(nmz_ed_align_plan *p, hipStream_t st, const uint64_t *d_off, const uint64_t *d_sym,
                  const uint32_t *d_pairs, uint64_t n_pairs, uint32_t *d_dist, nmz_edit_op *d_ops);

}  // namespace nmz
