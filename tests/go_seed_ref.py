"""Reference for the Go-seed reduction of the random policy's sweeps (helper, not a test file): a plain-Python
restatement of go_seed_from_table (namazu_amd/csrc/random_dev.h) in Python integers, so that nothing wraps unless it
is masked here, and Go's own rule over the oracle's 64-bit hash. Nothing here calls the library under test.

The sweeps never form u = FNV1a64(le64(seed) || le64(evhash)). With h0 the FNV state after le64(seed) and
L = h0 & 0xff, the xor of the first event byte touches only the low byte, so u = H + C (mod 2^64) with
H = h0 * P^8 and C = fnv8(L, evhash) - L * P^8; int64(u) mod M31 then follows from the residues of H and C and
from k = carry + sign, since 2^64 mod M31 = 4."""
from oracle import oracle as O

M31 = (1 << 31) - 1
M64 = (1 << 64) - 1
FNV_OFFSET = 0xCBF29CE484222325
FNV_PRIME = 0x100000001B3
P8 = pow(FNV_PRIME, 8, 1 << 64)
ZERO_SEED = 89482311

# the fixture's classes (tools/find_go_seed_edges.c): k, the pre-fold sum s1 or the post-fold value t, the Go seed
CLASSES = {
    "k0_s1_m31m1": dict(k=0, s1=M31 - 1, go_seed=M31 - 1),
    "k0_s1_m31": dict(k=0, s1=M31, go_seed=ZERO_SEED),
    "k0_s1_m31p1": dict(k=0, s1=M31 + 1, go_seed=1),
    "k1_s1_m31": dict(k=1, s1=M31, go_seed=M31 - 4),
    "k1_t3": dict(k=1, t=3, go_seed=M31 - 1),
    "k1_t4": dict(k=1, t=4, go_seed=ZERO_SEED),
    "k1_t5": dict(k=1, t=5, go_seed=1),
    "k2_s1_m31": dict(k=2, s1=M31, go_seed=M31 - 8),
    "k2_t7": dict(k=2, t=7, go_seed=M31 - 1),
    "k2_t8": dict(k=2, t=8, go_seed=ZERO_SEED),
    "k2_t9": dict(k=2, t=9, go_seed=1),
}


def fnv8(h, v):
    """FNV-1a 64 from state h over the 8 little-endian bytes of v"""
    for i in range(8):
        h = ((h ^ ((v >> (8 * i)) & 0xFF)) * FNV_PRIME) & M64
    return h


def go_reduce(seed):
    """rngSource.Seed: seed % int32max (Go's %: the sign of the dividend), + int32max if negative, 0 -> 89482311"""
    s = abs(seed) % M31
    if seed < 0:
        s = -s
    if s < 0:
        s += M31
    return ZERO_SEED if s == 0 else s


def residues(hm, cm, k):
    """The kernel's arithmetic from s1 = hm + cm on -> (s, s1, t, folded, borrowed, zero)"""
    s1 = hm + cm
    folded = s1 >= M31
    t = s1 - M31 if folded else s1
    borrowed = t < 4 * k
    s = t - 4 * k + (M31 if borrowed else 0)
    zero = s == 0
    return (ZERO_SEED if zero else s), s1, t, folded, borrowed, zero


def decompose(seed, evhash):
    """-> (u, H, C) with u the true hash and H + C = u (mod 2^64)"""
    h0 = fnv8(FNV_OFFSET, seed & M64)
    low = h0 & 0xFF
    H = (h0 * P8) & M64
    C = (fnv8(low, evhash) - low * P8) & M64
    return fnv8(h0, evhash), H, C


def table_seed(seed, evhash):
    """-> (s, k, carry, sign, s1, folded, borrowed, zero) as go_seed_from_table computes them"""
    _, H, C = decompose(seed, evhash)
    u = H + C  # not masked: bit 64 is the wrap
    carry = u >> 64
    u &= M64
    sign = u >> 63
    k = carry + sign
    s, s1, _, folded, borrowed, zero = residues(H % M31, C % M31, k)
    return s, k, carry, sign, s1, folded, borrowed, zero


def direct_seed(seed, evhash):
    """Go's rule applied to the oracle's int64(FNV1a64(le64(seed) || le64(evhash)))"""
    return go_reduce(O.random_event_seed(seed & M64, evhash))
