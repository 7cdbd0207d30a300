// xflow-amd: atof of a bounded byte range, correctly rounded for every input
// (the device text parser's number reader, kernels_parse.hip).  Host + device,
// so a CPU program can compare it with the C library's strtod.
#pragma once

#include <stdint.h>
#include <string.h>

#include <cmath>

#if defined(__HIPCC__)
#define XF_ATOF_HD __host__ __device__
#define XF_ATOF_SLOW __host__ __device__ __noinline__
#else
#define XF_ATOF_HD inline
#define XF_ATOF_SLOW inline
#endif

namespace xflow {

XF_ATOF_HD bool atof_space(char c) { return c == ' ' || (c >= '\t' && c <= '\r'); }

// The digits (and at most one '.') of [p, e) times 10^exp10, rounded to the
// nearest double, ties to even -- exact integer arithmetic on 32-bit limbs:
// digits * 5^d (or a quotient digits * 2^s / 5^-d with >= 65 bits and a sticky
// remainder), then one rounding to the 53 (subnormal: fewer) bits of the
// result.  At most 63 digits and |value| within 1e-324 .. 1e310 reach the
// limbs: 40 hold them (63 digits < 2^210, 5^393 < 2^913, 66 spare bits).
// The rare path: more than 15 significant digits or a decimal exponent
// beyond +-22.
XF_ATOF_SLOW double atof_big(const char* p, const char* e, int exp10) {
  constexpr int W = 40;
  uint32_t x[W];
  for (int i = 0; i < W; ++i) x[i] = 0u;
  int len = 1;
  auto mul_add = [&](uint32_t m, uint32_t a) {
    uint64_t carry = a;
    for (int i = 0; i < len; ++i) {
      const uint64_t t = (uint64_t)x[i] * m + carry;
      x[i] = (uint32_t)t;
      carry = t >> 32;
    }
    if (carry && len < W) x[len++] = (uint32_t)carry;
  };
  int nd = 0, frac = 0;
  bool dot = false;
  for (; p < e; ++p) {
    if (*p == '.') {
      dot = true;
      continue;
    }
    if (nd >= 63) break;  // (a caller's range holds at most 63 bytes)
    mul_add(10u, (uint32_t)(*p - '0'));
    nd += nd > 0 || *p != '0';
    frac += dot;
  }
  if (nd == 0) return 0.0;
  const int dex = exp10 - frac;
  const int mag = nd + dex;  // 10^(mag-1) <= value < 10^mag
  if (mag > 310) return INFINITY;
  if (mag < -323) return 0.0;  // (below half the smallest subnormal)
  constexpr uint32_t k5_13 = 1220703125u;  // 5^13
  auto pow5 = [](int k) {
    uint32_t r = 1u;
    for (int i = 0; i < k; ++i) r *= 5u;
    return r;
  };
  auto shift_left = [&](int s) {
    const int ws = s >> 5, bs = s & 31;
    for (int i = len - 1; i >= 0; --i) {
      x[i + ws] = x[i];
      if (ws) x[i] = 0u;
    }
    len += ws;
    if (bs) mul_add(1u << bs, 0u);
  };
  int e2;  // value = x * 2^e2 (+ sticky)
  bool sticky = false;
  if (dex >= 0) {
    for (int k = dex; k > 0; k -= 13) mul_add(k >= 13 ? k5_13 : pow5(k), 0u);
    shift_left(64);
    e2 = dex - 64;
  } else {
    const int k = -dex;
    const int s = ((k * 2379) >> 10) + 2 + 66;  // >= bits of 5^k, + 66
    shift_left(s);
    for (int j = k; j > 0; j -= 13) {
      const uint32_t d = j >= 13 ? k5_13 : pow5(j);
      uint64_t rem = 0;
      for (int i = len - 1; i >= 0; --i) {
        const uint64_t t = (rem << 32) | x[i];
        x[i] = (uint32_t)(t / d);
        rem = t % d;
      }
      sticky |= rem != 0;
      while (len > 1 && x[len - 1] == 0u) --len;
    }
    e2 = -k - s;
  }
  while (len > 1 && x[len - 1] == 0u) --len;
  int top = 31;
  while (!(x[len - 1] >> top)) --top;
  const int B = 32 * (len - 1) + top + 1;  // bits of x (>= 65)
  const int E = B - 1 + e2;                // 2^E <= value < 2^(E+1)
  if (E > 1023) return INFINITY;
  const int prec = E >= -1022 ? 53 : E + 1075;  // bits the result keeps
  if (prec < 0) return 0.0;
  const int lo = B - 64, w = lo >> 5, b = lo & 31;
  uint64_t t64 = (uint64_t)x[w] | ((uint64_t)x[w + 1] << 32);
  if (b) t64 = (t64 >> b) | ((uint64_t)x[w + 2] << (64 - b));
  for (int i = 0; i < w; ++i) sticky |= x[i] != 0u;
  if (b) sticky |= (x[w] & ((1u << b) - 1u)) != 0u;
  uint64_t kept = prec > 0 ? t64 >> (64 - prec) : 0ull;
  const bool half = (t64 >> (63 - prec)) & 1ull;
  sticky |= (t64 & ((1ull << (63 - prec)) - 1ull)) != 0ull;
  if (half && (sticky || (kept & 1ull))) ++kept;
  // (kept holds the implicit bit: it carries into the exponent field, and a
  // subnormal that rounds up to 2^-1022 becomes the smallest normal)
  const uint64_t bits = E >= -1022 ? ((uint64_t)(E + 1022) << 52) + kept : kept;
  if (bits >= 0x7FF0000000000000ull) return INFINITY;
  double r;
  memcpy(&r, &bits, sizeof(r));
  return r;
}

// atof of the NUL-terminated copy of [b, e) (reader.cpp range_atof: at most
// 63 characters, ends at a NUL byte): leading white space, sign, inf / nan,
// decimal digits with a fraction and an exponent.  Correctly rounded like
// glibc's strtod: up to 15 significant digits with |decimal exponent| <= 22
// are one exact product or quotient, the rest goes through atof_big.
// Hexadecimal floats are not recognised (they read as the 0 before the x).
XF_ATOF_HD double range_atof_exact(const char* b, const char* e) {
  if (e - b > 63) e = b + 63;
  const char* p = b;
  while (p < e && atof_space(*p)) ++p;
  bool neg = false;
  if (p < e && (*p == '+' || *p == '-')) neg = *p++ == '-';
  if (e - p >= 3 && (p[0] | 32) == 'i' && (p[1] | 32) == 'n' && (p[2] | 32) == 'f')
    return neg ? -INFINITY : INFINITY;
  if (e - p >= 3 && (p[0] | 32) == 'n' && (p[1] | 32) == 'a' && (p[2] | 32) == 'n') return NAN;
  const char* m0 = p;  // the digits and the '.'
  unsigned long long mant = 0;
  int digits = 0, ex = 0;
  bool any = false, cut = false;
  for (; p < e && *p >= '0' && *p <= '9'; ++p) {
    any = true;
    if (digits < 19) {
      mant = mant * 10ull + (unsigned long long)(*p - '0');
      digits += mant != 0ull;
    } else {
      cut = true;
    }
  }
  if (p < e && *p == '.') {
    for (++p; p < e && *p >= '0' && *p <= '9'; ++p) {
      any = true;
      if (digits < 19) {
        mant = mant * 10ull + (unsigned long long)(*p - '0');
        digits += mant != 0ull;
        --ex;
      } else {
        cut = true;
      }
    }
  }
  if (!any) return 0.0;
  const char* m1 = p;
  int ev = 0;
  if (p < e && (*p | 32) == 'e') {
    const char* q = p + 1;
    bool eneg = false;
    if (q < e && (*q == '+' || *q == '-')) eneg = *q++ == '-';
    for (; q < e && *q >= '0' && *q <= '9'; ++q) ev = ev < 100000 ? ev * 10 + (*q - '0') : ev;
    if (eneg) ev = -ev;
  }
  double r = (double)mant;
  ex += ev;
  if (mant != 0ull && (cut || mant > (1ull << 53) || ex > 22 || ex < -22)) {
    r = atof_big(m0, m1, ev);
  } else if (mant != 0ull && ex != 0) {
    double p10 = 1.0;  // (10^k, k <= 22: exact)
    for (int k = ex < 0 ? -ex : ex; k > 0; --k) p10 *= 10.0;
    r = ex > 0 ? r * p10 : r / p10;
  }
  return neg ? -r : r;
}

}  // namespace xflow
