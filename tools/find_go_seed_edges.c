/* Test-vector search (test infrastructure): event hashes at the edges of the Go-seed reduction that the random
 * policy's sweeps use (go_seed_from_table, namazu_amd/csrc/random_dev.h). The sweeps never
 * form u = FNV1a64(le64(seed) || le64(evhash)); they reduce int64(u) mod M31 = 2^31 - 1 from
 *   h0 = FNV prefix over le64(seed), L = h0 & 0xff, H = h0 * P^8, C = fnv8(L, evhash) - L * P^8  (H + C = u),
 *   Hm = H mod M31, Cm = C mod M31, k = carry + sign = (u < H) + (u >> 63)   (2^64 mod M31 = 4),
 *   s1 = Hm + Cm, t = s1 - M31 if s1 >= M31 else s1 (the fold), s = t - 4k (+ M31 on a borrow), 0 -> 89482311.
 * Each correction fires about once in 2^31 decisions, so the vectors are found by search. Classes:
 *   k0_s1_m31m1  k = 0, s1 = M31 - 1: no fold, s = M31 - 1      k1_s1_m31  k = 1, s1 = M31: fold, borrow, s = M31 - 4
 *   k0_s1_m31    k = 0, s1 = M31: folds to 0, s = 89482311      k1_t3      k = 1, t = 3: borrow, s = M31 - 1
 *   k0_s1_m31p1  k = 0, s1 = M31 + 1: s = 1                     k1_t4      k = 1, t = 4: s = 89482311
 *   k2_s1_m31    k = 2, s1 = M31: fold, borrow, s = M31 - 8     k1_t5      k = 1, t = 5: s = 1
 *   k2_t7 / k2_t8 / k2_t9   k = 2, t = 7 (borrow, s = M31 - 1), 8 (s = 89482311), 9 (s = 1)
 * H is fixed by the policy seed: H < 2^63 reaches k in {0, 1}, H >= 2^63 reaches k in {1, 2}; so two seeds. Both
 * have Hm > 9, so all their t classes fold (s1 = M31 + t); a t class that does not fold has s1 = t, which takes a
 * seed with Hm <= t: a third seed, with Hm = 0 and H >= 2^63, reaches t = 3, 4, 5 (k = 1) and 7, 8, 9 (k = 2)
 * unfolded and none of the other classes.
 * For one policy seed the tool walks evhash = splitmix(i), i < n, checks H + C == u on every candidate, and
 * prints, per (class, carry, sign), the `want` hits of smallest i as JSON lines (deterministic for given
 * arguments) with fields seed, evhash, k, carry, sign, s1, t, go_seed, class. go_seed is Go's own rule applied
 * to int64(u) and is checked against the decomposition on every hit.
 * `find_go_seed_edges scan lo hi` lists, for the seeds in [lo, hi), the ones whose H is nearest 2^62 and
 * 3 * 2^62 (where carry-only, sign-only and k = 0 or 2 are all likely), and every seed with Hm <= 9.
 * Build: gcc -O2 -fopenmp tools/find_go_seed_edges.c -o find_go_seed_edges
 * tests/golden/go_seed_edges.json is the output of
 *   find_go_seed_edges 2581 48000000000; find_go_seed_edges 7153 48000000000;
 *   find_go_seed_edges 735232460 20000000000
 * as the "vectors" list (about 4 minutes per 48e9 candidates on 8 cores; the seeds are from
 * `find_go_seed_edges scan 2048 10000` and `scan 2048 4294967296`). */
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define M31 2147483647ULL
static const uint64_t FNV_PRIME = 0x100000001b3ULL, FNV_OFFSET = 0xcbf29ce484222325ULL;

static uint64_t splitmix(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

/* FNV-1a over the 8 little-endian bytes of v, from state h */
static inline uint64_t fnv8(uint64_t h, uint64_t v) {
    for (int i = 0; i < 8; i++) h = (h ^ ((v >> (8 * i)) & 0xff)) * FNV_PRIME;
    return h;
}

static uint64_t pow8(void) {
    uint64_t p = 1;
    for (int i = 0; i < 8; i++) p *= FNV_PRIME;
    return p;
}

/* Go: seed % int32max; += int32max if negative; 0 -> 89482311 */
static uint32_t go_reduce(int64_t seed) {
    int64_t s = seed % (int64_t)M31;
    if (s < 0) s += (int64_t)M31;
    if (s == 0) s = 89482311;
    return (uint32_t)s;
}

enum { K0_M31M1, K0_M31, K0_M31P1, K1_M31, K1_T3, K1_T4, K1_T5, K2_M31, K2_T7, K2_T8, K2_T9, N_CLASSES };
static const char *CLASS_NAME[N_CLASSES] = {"k0_s1_m31m1", "k0_s1_m31", "k0_s1_m31p1", "k1_s1_m31", "k1_t3", "k1_t4",
                                            "k1_t5",       "k2_s1_m31", "k2_t7",       "k2_t8",     "k2_t9"};

typedef struct {
    uint64_t i, evhash, s1;
    uint32_t k, carry, sign, t, go_seed;
    int cls;
} hit_t;

static int by_index(const void *a, const void *b) {
    const uint64_t x = ((const hit_t *)a)->i, y = ((const hit_t *)b)->i;
    return x < y ? -1 : x > y;
}

static int scan(uint64_t lo, uint64_t hi) {
    const uint64_t P8 = pow8(), target[2] = {1ULL << 62, 3ULL << 62};
    for (int w = 0; w < 2; w++) {
        uint64_t best = 0, best_d = UINT64_MAX;
        for (uint64_t seed = lo; seed < hi; seed++) {
            const uint64_t H = fnv8(FNV_OFFSET, seed) * P8;
            const uint64_t d = H > target[w] ? H - target[w] : target[w] - H;
            if (d < best_d) best_d = d, best = seed;
        }
        printf("seed %" PRIu64 ": H = 0x%016" PRIx64 "\n", best, fnv8(FNV_OFFSET, best) * P8);
    }
    /* a t class that did not fold has s1 = t <= 9, so Hm <= t: about one seed in 2^28 */
#pragma omp parallel for schedule(static)
    for (uint64_t seed = lo; seed < hi; seed++) {
        const uint64_t H = fnv8(FNV_OFFSET, seed) * P8;
        if (H % M31 <= 9)
#pragma omp critical
            printf("seed %" PRIu64 ": H = 0x%016" PRIx64 ", Hm = %u\n", seed, H, (unsigned)(H % M31));
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 3 && !strcmp(argv[1], "scan")) return scan(strtoull(argv[2], 0, 0), strtoull(argv[3], 0, 0));
    if (argc < 3) {
        fprintf(stderr, "usage: %s seed n_candidates [want per (class, carry, sign)] | scan lo hi\n", argv[0]);
        return 2;
    }
    const uint64_t seed = strtoull(argv[1], 0, 0), n = strtoull(argv[2], 0, 0);
    const int want = argc > 3 ? atoi(argv[3]) : 1;
    const uint64_t P8 = pow8(), h0 = fnv8(FNV_OFFSET, seed), L = h0 & 0xff, H = h0 * P8, LP8 = L * P8;
    const uint32_t Hm = (uint32_t)(H % M31);
    fprintf(stderr, "seed %" PRIu64 ": H = 0x%016" PRIx64 " (k in {%s}), Hm = %u, L = %u\n", seed, H,
            H >> 63 ? "1, 2" : "0, 1", Hm, (unsigned)L);
    enum { MAX_HITS = 4096 };
    static hit_t hits[MAX_HITS];
    int n_hits = 0, bad = 0;
#pragma omp parallel for schedule(static)
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t eh = splitmix(i);
        const uint64_t u = fnv8(h0, eh);          /* the true hash */
        const uint64_t C = fnv8(L, eh) - LP8;     /* the table entry of row L */
        if (H + C != u) {
#pragma omp atomic write
            bad = 1;
            continue;
        }
        const uint32_t Cm = (uint32_t)(C % M31);
        const uint32_t carry = u < H, sign = (uint32_t)(u >> 63), k = carry + sign;
        const uint64_t s1 = (uint64_t)Hm + Cm;
        const uint32_t t = (uint32_t)(s1 >= M31 ? s1 - M31 : s1);
        int cls = -1;
        if (s1 == M31)
            cls = k == 0 ? K0_M31 : k == 1 ? K1_M31 : K2_M31;
        else if (k == 0 && s1 == M31 - 1)
            cls = K0_M31M1;
        else if (k == 0 && s1 == M31 + 1)
            cls = K0_M31P1;
        else if (k == 1 && t >= 3 && t <= 5)
            cls = K1_T3 + (int)(t - 3);
        else if (k == 2 && t >= 7 && t <= 9)
            cls = K2_T7 + (int)(t - 7);
        if (cls < 0) continue;
        uint32_t s = t >= 4 * k ? t - 4 * k : t - 4 * k + (uint32_t)M31;
        if (s == 0) s = 89482311;
#pragma omp critical
        {
            if (s != go_reduce((int64_t)u)) bad = 1;
            if (n_hits < MAX_HITS)
                hits[n_hits++] = (hit_t){i, eh, s1, k, carry, sign, t, s, cls};
        }
    }
    if (bad) {
        fprintf(stderr, "the decomposition disagreed with the direct form\n");
        return 1;
    }
    qsort(hits, (size_t)n_hits, sizeof hits[0], by_index);
    int count[N_CLASSES][2][2] = {{{0}}};
    for (int j = 0; j < n_hits; j++) {
        const hit_t *h = &hits[j];
        if (count[h->cls][h->carry][h->sign]++ >= want) continue;
        printf("{\"seed\": %" PRIu64 ", \"evhash\": %" PRIu64 ", \"k\": %u, \"carry\": %u, \"sign\": %u, \"s1\": %" PRIu64
               ", \"t\": %u, \"go_seed\": %u, \"class\": \"%s\"}\n",
               seed, h->evhash, h->k, h->carry, h->sign, h->s1, h->t, h->go_seed, CLASS_NAME[h->cls]);
    }
    for (int c = 0; c < N_CLASSES; c++)
        fprintf(stderr, "%-12s %d hit(s)\n", CLASS_NAME[c],
                count[c][0][0] + count[c][0][1] + count[c][1][0] + count[c][1][1]);
    return 0;
}
