/* Test-vector search (test infrastructure): ProcSetEvent decisions in which one sub-policy draw is rejected by
 * Go's Int31n bound in mid-sequence, under the random policy's per-event seeding:
 *   dirichlet_mid   dirichlet, 500 processes: an Intn(999) draw (1.3e-7 per draw)
 *   extreme_mark    extreme, 410 processes, prioritized 256: an Int31n(410) mark draw (1.9e-7 per draw)
 *   mild_mid        mild, 512 processes: an Int31n(40) draw (3.7e-9 per draw)
 *   extreme_prio    extreme, 512 processes, prioritized 256: an Int31n(10) priority draw (3.7e-9 per draw)
 * all with a ranged interval 30-100 ms (one accepted Int63n delay draw first). Uses the CPU oracle's generator
 * (oracle/nmz_oracle.c): a draw that consumes more than one output was rejected. A vector has exactly one
 * rejected draw, not the first sub-policy draw, so its decision consumes one output more than it has draws.
 * Output: JSON lines for tests/golden/procset_rejections.json; "draw" is the rejected draw's index in the
 * decision (the delay draw is draw 0), "outputs" the generator outputs the decision consumes.
 * Build: gcc -O2 -fopenmp tools/find_procset_rejections.c -Loracle/build -lnmz_oracle -o find_procset_rejections
 * Run:   find_procset_rejections [seed [max events per case [vectors per case [seconds per case]]]] */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <omp.h>

typedef struct nmzo_go_rng {
    int tap, feed;
    int64_t n_out;
    uint64_t vec[607];
} nmzo_go_rng;

void nmzo_init(void);
void nmzo_go_seed(nmzo_go_rng *rng, int64_t seed);
int64_t nmzo_go_int63n(nmzo_go_rng *rng, int64_t n);
int32_t nmzo_go_int31n(nmzo_go_rng *rng, int32_t n);
int64_t nmzo_random_event_seed(uint64_t seed, uint64_t evhash);

static uint64_t splitmix(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

enum { DIRICHLET_MID, EXTREME_MARK, MILD_MID, EXTREME_PRIO, N_CASES };
static const struct {
    const char *name, *policy;
    int n_procs, prioritized;
} CASES[N_CASES] = {{"dirichlet_mid", "dirichlet", 500, 3},
                    {"extreme_mark", "extreme", 410, 256},
                    {"mild_mid", "mild", 512, 3},
                    {"extreme_prio", "extreme", 512, 256}};
#define MIN_NS 30000000LL
#define MAX_NS 100000000LL

/* one draw; returns its value, counts it, and records its index when it consumed more than one output */
static int32_t draw31n(nmzo_go_rng *r, int32_t n, int *n_draws, int *n_rej, int *rej_at) {
    const int64_t before = r->n_out;
    const int32_t v = nmzo_go_int31n(r, n);
    if (r->n_out - before > 1) {
        *n_rej += (int)(r->n_out - before - 1);
        *rej_at = *n_draws;
    }
    ++*n_draws;
    return v;
}

/* the decision of one event; returns 1 when it is a vector of case c */
static int try_event(int c, uint64_t seed, uint64_t eh, int *draw, int *outputs) {
    nmzo_go_rng r;
    nmzo_go_seed(&r, nmzo_random_event_seed(seed, eh));
    int n_draws = 1, n_rej = 0, rej_at = -1, first = 1, lo = 0, hi = 0;
    (void)nmzo_go_int63n(&r, MAX_NS - MIN_NS);
    if (r.n_out != 1) return 0; /* the delay draw itself was re-drawn */
    const int n = CASES[c].n_procs;
    if (c == DIRICHLET_MID || c == MILD_MID) {
        for (int i = 0; i < n; i++) (void)draw31n(&r, c == MILD_MID ? 40 : 999, &n_draws, &n_rej, &rej_at);
        lo = first + 1, hi = n_draws;
    } else {
        static _Thread_local unsigned char mark[512];
        memset(mark, 0, sizeof mark);
        for (int j = 0; j < CASES[c].prioritized; j++) mark[draw31n(&r, n, &n_draws, &n_rej, &rej_at)] = 1;
        const int phase2 = n_draws;
        for (int i = 0; i < n; i++)
            if (mark[i]) (void)draw31n(&r, 10, &n_draws, &n_rej, &rej_at);
        if (c == EXTREME_MARK)
            lo = first + 1, hi = phase2;
        else
            lo = phase2, hi = n_draws;
    }
    if (n_rej != 1 || rej_at < lo || rej_at >= hi) return 0;
    *draw = rej_at;
    *outputs = (int)r.n_out;
    return 1;
}

int main(int argc, char **argv) {
    const uint64_t seed = argc > 1 ? strtoull(argv[1], 0, 0) : 0x5EED;
    const uint64_t n = argc > 2 ? strtoull(argv[2], 0, 0) : 40000000ULL;
    const int want = argc > 3 ? atoi(argv[3]) : 2;
    const double limit = argc > 4 ? atof(argv[4]) : 120.0;
    nmzo_init();
    for (int c = 0; c < N_CASES; c++) {
        int found = 0;
        const double t0 = omp_get_wtime();
#pragma omp parallel for schedule(dynamic, 4096)
        for (uint64_t i = 0; i < n; i++) {
            if (found >= want || omp_get_wtime() - t0 > limit) continue;
            const uint64_t eh = splitmix(i);
            int draw, outputs;
            if (!try_event(c, seed, eh, &draw, &outputs)) continue;
#pragma omp critical
            if (found < want) {
                found++;
                printf("{\"case\": \"%s\", \"seed\": %llu, \"evhash\": %llu, \"policy\": \"%s\", \"use_batch\": 1, "
                       "\"prioritized\": %d, \"reset_probability\": 0.1, \"min_ns\": %lld, \"max_ns\": %lld, "
                       "\"n_procs\": %d, \"draw\": %d, \"outputs\": %d}\n",
                       CASES[c].name, (unsigned long long)seed, (unsigned long long)eh, CASES[c].policy,
                       CASES[c].prioritized, MIN_NS, MAX_NS, CASES[c].n_procs, draw, outputs);
                fflush(stdout);
            }
        }
        fprintf(stderr, "%s: %d vector(s) in %.1f s\n", CASES[c].name, found, omp_get_wtime() - t0);
    }
    return 0;
}
