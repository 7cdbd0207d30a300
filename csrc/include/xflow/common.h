// xflow-amd: shared host/device definitions.
//
// Everything in this header is usable from both the C++ CPU backend and the
// gfx950 HIP kernels.  It holds the per-element math that defines reference
// behaviour (sigmoid clamps, FTRL-Proximal closed form, SGD) so that both
// backends execute bit-for-bit the same scalar recipe.
//
// Reference semantics:
//   sigmoid            /root/reference/src/base/base.h:54-63
//   FTRL-Proximal      /root/reference/src/optimizer/ftrl.h:58-74 (w), :125-141 (v)
//   SGD                /root/reference/src/optimizer/sgd.h:50-52, :94-96
//   v lazy init        /root/reference/src/optimizer/ftrl.h:114-120 (N(0,1)*1e-2)
#pragma once

#include <stdint.h>
#include <math.h>

#if defined(__HIPCC__)
#define XF_HD __host__ __device__ __forceinline__
#else
#define XF_HD inline
#endif

namespace xflow {

using u64 = uint64_t;
using u32 = uint32_t;

// Slot sentinel for every open-addressing table.  A user key equal to the
// sentinel is remapped to kEmptyKey-1 (documented in docs/DESIGN.md).
constexpr u64 kEmptyKey = ~0ull;

XF_HD u64 sanitize_key(u64 k) { return k == kEmptyKey ? kEmptyKey - 1 : k; }

// 64-bit finaliser (murmur3 fmix64).  Low bits index table slots, the high
// 32 bits choose the owning rank, so the two are independent.
XF_HD u64 fmix64(u64 h) {
  h ^= h >> 33;
  h *= 0xff51afd7ed558ccdull;
  h ^= h >> 33;
  h *= 0xc4ceb9fe1a85ec53ull;
  h ^= h >> 33;
  return h;
}

// Row shuffling (Backend::shuffle_rows, docs/DESIGN.md §9): a keyed bijection
// of [0, n) that needs no memory and no sort, so every lane computes its own
// pi(i).  A 4-round Feistel network over the 2h-bit domain 2^(2h) >= n
// (h = half the bit length of n - 1, rounded up; the domain is below 4n),
// cycle-walked back into [0, n): a pass maps the domain onto itself one to
// one, so repeating it from i until the value falls below n is a bijection
// of [0, n) (the walk from i < n returns to i at the latest, so it ends).
// Round keys k_r = fmix64(seed + 0x9E3779B97F4A7C15 * (r + 1)), r = 0..3;
// one pass: L = x >> h, R = x & mask; four times (L, R) = (R, (L ^ fmix64(R ^
// k_r)) & mask); x = L << h | R.  Well mixed at block sizes (thousands of
// rows), not uniform over all permutations at tiny n.
constexpr int kShuffleRounds = 4;
struct ShufflePerm {
  u64 n = 0, mask = 0;
  int h = 0;
  u64 k[kShuffleRounds] = {};
  XF_HD u64 at(u64 i) const {
    if (n <= 1) return i;
    u64 x = i;
    do {
      u64 L = x >> h, R = x & mask;
      for (int r = 0; r < kShuffleRounds; ++r) {
        const u64 t = (L ^ fmix64(R ^ k[r])) & mask;
        L = R;
        R = t;
      }
      x = (L << h) | R;
    } while (x >= n);
    return x;
  }
};
XF_HD ShufflePerm shuffle_perm(u64 n, u64 seed) {
  ShufflePerm p;
  p.n = n;
  if (n <= 1) return p;
  const int b = 64 - __builtin_clzll(n - 1);  // bit length of n - 1
  p.h = (b + 1) / 2 < 1 ? 1 : (b + 1) / 2;
  p.mask = (1ull << p.h) - 1;
  for (int r = 0; r < kShuffleRounds; ++r)
    p.k[r] = fmix64(seed + 0x9E3779B97F4A7C15ull * (u64)(r + 1));
  return p;
}
// pi(i): the source row of destination row i
XF_HD u64 shuffle_index(u64 i, u64 n, u64 seed) { return shuffle_perm(n, seed).at(i); }

// Feature crosses (Backend::cross_rows, docs/DESIGN.md §9): the key of the
// cross of m fields (2..4, in the spec's order) whose operands in a row are
// ops[i] -- the row's raw key of field fields[i], or ~0 when the row has none:
// a missing operand is hashed like any other value, so every row gets a key.
// The salt keeps cross keys apart from every other use of fmix64 here; the
// arity and the field ids are hashed in, so 3x7, 7x3 and 3x7x1 never share
// keys by construction.  Mirrored in xflow_amd/engine.py (cross_keys).
constexpr u64 kCrossSalt = 0xC3A5C85C97CB3127ull;
XF_HD u64 cross_key(const int32_t* fields, const u64* ops, int m) {
  u64 h = fmix64(kCrossSalt + (u64)m);
  for (int i = 0; i < m; ++i) {
    h = fmix64(h ^ (u64)(u32)fields[i]);
    h = fmix64(h ^ ops[i]);
  }
  return sanitize_key(h);
}

// Synthetic "historic" key i of a prefilled table (Backend::table_prefill):
// bit 62 set, so it never equals a hashed feature below 2^62.
XF_HD u64 prefill_key(u64 seed, u64 i) {
  return (1ull << 62) | (fmix64(seed * 0x9E3779B97F4A7C15ull + i) >> 2);
}

XF_HD u32 owner_of(u64 key, u32 world) {
  return world <= 1 ? 0u : (u32)((fmix64(key) >> 32) % world);
}

// Feature admission (EngineConfig::admit_min_count, docs/DESIGN.md §2): where
// a key counts its sightings in the blocked counting filter of 2^log2 bytes.
// One fmix64 of the key, salted so that it is independent of the key's table
// home and owner, gives from disjoint bits two distinct byte offsets inside
// one 64-byte block (bits 0-5 and 6-11; equal offsets: the second is the
// first ^ 1) and the block (bits 12 and up).  An absent key costs one random
// line.  Mirrored in xflow_amd/testing/hashing.py.
constexpr u64 kAdmitSalt = 0xa0761d6478bd642full;
constexpr int kAdmitBlockLog2 = 6;
constexpr int kAdmitMaxLog2 = 32;
struct AdmitPos {
  u64 c0, c1;  // byte indices of the key's two counters
};
XF_HD AdmitPos admit_pos(u64 key, int log2_bytes) {
  const u64 h = fmix64(key ^ kAdmitSalt);
  const u64 o0 = h & 63u;
  u64 o1 = (h >> 6) & 63u;
  if (o1 == o0) o1 = o0 ^ 1u;
  const u64 block = (h >> 12) & ((1ull << (log2_bytes - kAdmitBlockLog2)) - 1);
  AdmitPos p;
  p.c0 = (block << kAdmitBlockLog2) | o0;
  p.c1 = (block << kAdmitBlockLog2) | o1;
  return p;
}

// Delta checkpoints (EngineConfig::delta_track, docs/DESIGN.md §2): the bit of
// a key in the touched-key filter of 2^log2 bits.  Indexed by a salted hash
// of the key, not by its slot -- splits and prune re-pack slots -- and
// independent of the key's table home, owner and admission counters.  One bit
// per key: a collision can only add an untouched key to a delta.  Mirrored in
// xflow_amd/testing/hashing.py.
constexpr u64 kDeltaSalt = 0xe7037ed1a0b428dbull;
constexpr int kDeltaMinLog2 = 10;
constexpr int kDeltaMaxLog2 = 34;
XF_HD u64 delta_bit(u64 key, int log2_bits) {
  return fmix64(key ^ kDeltaSalt) & ((1ull << log2_bits) - 1);
}

// Reference sigmoid: clamp at |x|>30, otherwise e^x/(1+e^x) evaluated in
// double with the literal base 2.718281828 (base.h:54-63).
XF_HD float sigmoid_ref(float x) {
  if (x < -30.0f) return 1e-6f;
  if (x > 30.0f) return 1.0f;
  // pow(2.718281828, x) == exp(x * ln(2.718281828))
  const double kLnBase = 0.9999999998311266;  // ln(2.718281828)
  double ex = exp((double)x * kLnBase);
  return (float)(ex / (1.0 + ex));
}

// ---------------------------------------------------------------------------
// Optimizers.  The table stores per parameter either (n, z) [FTRL] or w [SGD].
// FTRL's weight is a pure function of (z, n) after the first push, so it is
// never stored: pull recomputes it with exactly the reference float recipe.
// ---------------------------------------------------------------------------
struct FtrlParams {
  float alpha = 5e-2f;    // ftrl.h:17
  float beta = 1.0f;      // ftrl.h:18
  float lambda1 = 5e-5f;  // ftrl.h:19
  float lambda2 = 10.0f;  // ftrl.h:20
};

// (sn = sqrtf(n): a chain of pushes onto one parameter carries it, so each
// push takes one square root instead of three -- the same floats)
// The reference divides by alpha twice per push (ftrl.h:62,69); here both
// are products with float(1 / alpha): a push's dependency chain (a hot key's
// slice-long chain of pushes is sequential by definition) keeps one IEEE
// division instead of three, within an ulp of the quotients.
XF_HD float ftrl_inv_alpha(const FtrlParams& p) { return 1.0f / p.alpha; }
XF_HD float ftrl_weight_sn(float z, float sn, const FtrlParams& p) {
  if (fabsf(z) <= p.lambda1) return 0.0f;
  float tmpr = 0.0f;
  if (z > 0.0f) tmpr = z - p.lambda1;
  if (z < 0.0f) tmpr = z + p.lambda1;
  float tmpl = -1.0f * ((p.beta + sn) * ftrl_inv_alpha(p) + p.lambda2);
  return tmpr / tmpl;
}

XF_HD float ftrl_weight(float z, float n, const FtrlParams& p) {
  return ftrl_weight_sn(z, sqrtf(n), p);
}

// One FTRL-Proximal push of gradient g onto (n, z) whose current weight is w.
XF_HD void ftrl_push_sn(float& n, float& z, float& sn, float w, float g, const FtrlParams& p) {
  float nn = n + g * g;
  float snn = sqrtf(nn);
  z += g - (snn - sn) * ftrl_inv_alpha(p) * w;
  n = nn;
  sn = snn;
}

XF_HD void ftrl_push(float& n, float& z, float w, float g, const FtrlParams& p) {
  float sn = sqrtf(n);
  ftrl_push_sn(n, z, sn, w, g, p);
}

struct SgdParams {
  float lr = 0.001f;      // sgd.h:16
  float v_init = 0.001f;  // sgd.h:69
};

// ---------------------------------------------------------------------------
// Deterministic lazy initialisation of latent (v) parameters: N(0,1)*scale,
// derived from (seed, key, dim) by a counter-based hash + Box-Muller.  The
// reference draws from a time-seeded default_random_engine (base.h:33-44), so
// any N(0,1) source is behaviour-equivalent; ours is reproducible and needs no
// RNG state, which lets any reader of an un-pushed slot materialise the value.
// ---------------------------------------------------------------------------
XF_HD float normal_init(u64 key, u32 dim, u64 seed) {
  u64 a = fmix64(key ^ (seed * 0x9e3779b97f4a7c15ull) ^ ((u64)dim << 48) ^ 0x243f6a8885a308d3ull);
  u64 b = fmix64(a ^ 0x13198a2e03707344ull);
  // 24-bit uniforms in (0,1]
  float u1 = ((float)(a >> 40) + 1.0f) * (1.0f / 16777216.0f);
  float u2 = ((float)(b >> 40)) * (1.0f / 16777216.0f);
  float r = sqrtf(-2.0f * logf(u1));
  return r * cosf(6.283185307179586f * u2);
}

}  // namespace xflow
