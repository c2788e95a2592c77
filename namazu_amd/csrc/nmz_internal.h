// Cross-translation-unit declarations inside libnmz_gpu.so.
#pragma once
#include "nmz_common.h"

namespace nmz {

uint64_t topk_scratch_entries(uint64_t n, uint32_t k);
int topk_merge_lists(hipStream_t st, nmz_topk_entry *a, nmz_topk_entry *b, uint64_t lists, uint32_t k,
                     nmz_topk_entry *d_out);
int topk_select(hipStream_t st, const nmz_sched_stats *d_stats, uint64_t n, uint64_t seed0, uint32_t k,
                nmz_topk_entry *d_scratch, nmz_topk_entry *d_out);

// scratch carving helper: bump allocator over one device buffer (256-B aligned)
struct Carve {
    char *base;
    size_t off = 0;
    explicit Carve(void *p) : base(static_cast<char *>(p)) {}
    template <typename T>
    T *take(size_t count) {
        T *p = reinterpret_cast<T *>(base + off);
        off += (count * sizeof(T) + 255) & ~size_t(255);
        return p;
    }
    static size_t bytes_for(size_t count, size_t elem) { return (count * elem + 255) & ~size_t(255); }
};

// unique.hip: sorted distinct symbols on the device (hipcub radix sort + unique); *n_uniq on the host
int device_unique_u64(const uint64_t *d_sym, uint64_t total, uint64_t *d_uniq, uint64_t cap, uint64_t *n_uniq,
                      hipStream_t st);
// unique.hip, for delivery.hip: the per-context table of the signature's rank keys (sig_dev.h; RANK_KEYS entries,
// built on first use), and the equality classes of d_sig[2 * N]: first[i] = the smallest j with sig_j == sig_i
// (radix sort with the index as payload; scratch ctx->buf[6]). The caller holds ctx.
int sig_rank_keys(nmz_ctx *ctx, const ulonglong2 **out);
int classes_launch(nmz_ctx *ctx, const uint64_t *d_sig, uint32_t N, uint32_t *d_first, hipStream_t st);

// match.hip, for contrast.hip (nmz_order_contrast_runs). match_validate: every limit of the host forms, no device.
int match_validate(const uint64_t *sym, const int64_t *arrival, uint32_t E, const uint64_t *run_off,
                   const uint64_t *run_sym, uint64_t n_runs);
// One host-form match on the context's stream; the caller holds ctx and has validated. run() builds the universe's
// plan, takes rows, offsets and symbols from the context's pool for the call, uploads the CSR and enqueues the
// match: *d_pos = the [n_runs][E] rows. The destructor drains the stream before plan and buffer go back.
struct MatchCall {
    nmz_ctx *ctx;
    nmz_match_plan *plan = nullptr;
    DevBuf work;
    explicit MatchCall(nmz_ctx *c) : ctx(c) { work.pool = &c->pool; }
    ~MatchCall();
    int run(const uint64_t *sym, const int64_t *arrival, uint32_t E, const uint64_t *run_off,
            const uint64_t *run_sym, uint64_t n_runs, uint32_t **d_pos);
};

}  // namespace nmz
