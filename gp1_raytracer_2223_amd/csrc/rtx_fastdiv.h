// rtx_fastdiv.h — cheap correctly rounded binary32 reciprocal / quotient for gfx950.
//
// hipcc's IEEE division a/b expands to ~11 VALU ops (v_div_scale x2, v_rcp, 4-5 FMAs,
// v_div_fmas, v_div_fixup) because it must handle every range.  Inside a checked domain
// the classic Markstein sequence gives the same correctly rounded result in 3 + 3 ops:
//   y  = v_rcp_f32(b);  e = fma(-b, y, 1);  y = fma(e, y, y)   -> RN(1/b)
//   q  = a * y;         r = fma(-b, q, a);  q = fma(r, y, q)    -> RN(a/b)
// RN(1/b) is verified EXHAUSTIVELY on the hardware for every b in the domain
// (tools/validate_fastdiv.hip, all 2^32 inputs), and the quotient step is Markstein's
// theorem (y = RN(1/b), q0 within 1 ulp, exact residual by FMA) — additionally checked
// on 2^33 random and near-halfway pairs by the same tool.  Lanes outside the domain
// (zeros, tiny or huge magnitudes, inf, NaN) take the IEEE `/` in a divergent branch that
// is skipped whenever no lane needs it.
#pragma once
#include <hip/hip_runtime.h>

namespace rtxd {

// |b| in [2^-60, 2^60]: RN(1/b) and every intermediate stay normal.
__device__ __forceinline__ bool fast_rcp_ok(float b) {
    const float ab = fabsf(b);
    return ab >= 0x1p-60f && ab <= 0x1p60f;
}

__device__ __forceinline__ float rcp_rn(float b) {
    const float y0 = __builtin_amdgcn_rcpf(b);
    const float e = fmaf(-b, y0, 1.0f);
    return fmaf(e, y0, y0);
}

// a == 0 or |a| in [2^-60, 2^60], and fast_rcp_ok(b): quotient in [2^-120, 2^120] and the
// residual a - b*q is exactly representable (granularity >= 2^-106).
__device__ __forceinline__ bool fast_num_ok(float a) {
    const float aa = fabsf(a);
    return (aa >= 0x1p-60f && aa <= 0x1p60f) || a == 0.0f;
}

__device__ __forceinline__ bool fast_div_ok(float a, float b) { return fast_num_ok(a) && fast_rcp_ok(b); }

// RN(a/b) given y = rcp_rn(b), inside the domain above.
__device__ __forceinline__ float div_rn(float a, float b, float y) {
    const float q = a * y;
    const float r = fmaf(-b, q, a);
    return fmaf(r, y, q);
}

// RN(1/b) for every b.
__device__ __forceinline__ float rcp_exact(float b) {
    float y = rcp_rn(b);
    if (__builtin_expect(!fast_rcp_ok(b), 0)) y = 1.f / b;
    return y;
}

// RN(1/x), RN(1/y), RN(1/z) with ONE domain test for the three: the IEEE fallback runs
// only in lanes where some component is outside.  Returns the ballot of those lanes.  In
// the domain every reciprocal is finite and non-zero, which is what the FAST slab path
// needs, so the ballot doubles as its (conservative) exclusion mask.  The magnitude sum
// carries a NaN or inf component into the test (v_min3 would drop a NaN).
__device__ __forceinline__ unsigned long long rcp3_exact(float x, float y, float z, float& rx, float& ry, float& rz) {
    rx = rcp_rn(x); ry = rcp_rn(y); rz = rcp_rn(z);
    const float lo = fminf(fminf(fabsf(x), fabsf(y)), fabsf(z));
    const float sum = (fabsf(x) + fabsf(y)) + fabsf(z);
    const bool in = lo >= 0x1p-60f && sum <= 0x1p60f;
    const unsigned long long out = __builtin_amdgcn_ballot_w64(!in);
    if (__builtin_expect(!in, 0)) {
        rx = 1.f / x; ry = 1.f / y; rz = 1.f / z;
    }
    return out;
}

// (x, y, z) / m, each correctly rounded, for m = |(x, y, z)| as computed by the caller.
__device__ __forceinline__ void div3_exact(float& x, float& y, float& z, float m) {
    const float r = rcp_rn(m);
    const float qx = div_rn(x, m, r), qy = div_rn(y, m, r), qz = div_rn(z, m, r);
    // a NaN component (dropped by v_min) gives NaN on both paths; inf makes m inf -> IEEE
    const float lo = fminf(fminf(fabsf(x), fabsf(y)), fabsf(z));
    if (__builtin_expect(!(fast_rcp_ok(m) && lo >= 0x1p-60f), 0)) {
        x = x / m; y = y / m; z = z / m;
    } else {
        x = qx; y = qy; z = qz;
    }
}

// RN(sqrt(x)) for x == 0, every x >= 2^-96 and +inf: v_sqrt_f32 (1 ulp) plus one residual
// correction against its two neighbours, without the denormal scaling and class handling of
// the correctly rounded sqrtf (7 VALU less).  Compared with sqrtf over all 2^31 non-negative
// inputs by tools/validate_sqrt.hip -DFAST=1 (profiles/r01/validate_sqrt_fast.txt,
// profiles/fixedpath/validate_sqrt_fast.txt): it differs only below 2^-96.  It has no domain
// test of its own: the caller's covers it (norm_ray3).
__device__ __forceinline__ float sqrt_rn(float x) {
    float s = __builtin_amdgcn_sqrtf(x);
    const float sm = __uint_as_float(__float_as_uint(s) - 1u), sp = __uint_as_float(__float_as_uint(s) + 1u);
    const float rm = fmaf(-sm, s, x), rp = fmaf(-sp, s, x);
    s = (rm <= 0.f) ? sm : s;
    s = (rp > 0.f) ? sp : s;
    return s;
}

// A ray direction in one piece: m = RN(sqrt(x*x + y*y + z*z)), (x, y, z) = RN((x, y, z) / m)
// (Vector3::Normalize) and r = RN(1 / (x, y, z)) of the normalised direction (dae::Ray's
// inversedDir), with ONE domain test and ONE wave-uniform fallback for the three steps, which
// sqrtf, div3_exact and rcp3_exact each guarded with a divergent region of their own.  The fast
// forms (sqrt_rn, div_rn, rcp_rn) are computed in every lane; a wave with a lane outside the
// domain recomputes that lane with the IEEE forms, which are right for any operand.
// The test, with s = x*x + y*y + z*z as computed, lo = min |component| before and dlo after
// the normalisation:   2^-96 <= s <= 2^120   and   lo >= 2^-60   and   dlo >= 2^-60.
//   * sqrt_rn: s >= 2^-96 is its domain (s is a sum of squares: never negative).
//   * div3_exact needs fast_rcp_ok(m) and lo >= 2^-60.  The square root is monotone and
//     sqrt(2^-96) = 2^-48, sqrt(2^120) = 2^60 are exact, so m lies in [2^-48, 2^60].  (Each
//     numerator is at most 2^60 too: a sum of non-negative terms rounds to no less than any of
//     them, and the square of the next float above 2^60 already rounds above 2^120.)
//   * rcp3_exact needs dlo >= 2^-60 and |x| + |y| + |z| <= 2^60 after the normalisation.  In the two
//     domains above every quotient is the correctly rounded one of |x| / m with m >= max |component|
//     (1 - 2u), so each is at most 1 + 3u and their sum below 4: the upper bound holds.
//   * a NaN component makes s NaN and an infinite one makes it inf: both fail the test on s (v_min3
//     would drop a NaN, but lo and dlo are read only once s has passed).
// Returns rcp3_exact's ballot: the lanes whose normalised direction is outside its domain.  In a
// wave that skips the fallback every lane is inside (the test implies it), so the ballot is 0; the
// fallback evaluates rcp3_exact's own condition on the final direction.
// ONE = false: the three guarded steps as they were (a kernel that the merged form costs a wave of occupancy).
template <bool ONE = true>
__device__ __forceinline__ unsigned long long norm_ray3(float& x, float& y, float& z, float& m, float& rx, float& ry,
                                                        float& rz) {
    if constexpr (!ONE) {
        m = sqrtf(x * x + y * y + z * z);
        div3_exact(x, y, z, m);
        return rcp3_exact(x, y, z, rx, ry, rz);
    }
    const float x0 = x, y0 = y, z0 = z;
    const float s = x0 * x0 + y0 * y0 + z0 * z0;
    m = sqrt_rn(s);
    const float r = rcp_rn(m);
    x = div_rn(x0, m, r); y = div_rn(y0, m, r); z = div_rn(z0, m, r);
    rx = rcp_rn(x); ry = rcp_rn(y); rz = rcp_rn(z);
    const float lo = fminf(fminf(fabsf(x0), fabsf(y0)), fabsf(z0));
    const float dlo = fminf(fminf(fabsf(x), fabsf(y)), fabsf(z));
    // (2^-96 <= s <= 2^120 on the bits, one unsigned compare: zero, a denormal, inf and NaN all fall outside)
    const bool in = (__float_as_uint(s) - 0x0f800000u <= 0x7b800000u - 0x0f800000u) && lo >= 0x1p-60f && dlo >= 0x1p-60f;
    unsigned long long slow = 0;
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(!in) != 0, 0)) {   // wave-uniform
        if (!in) {
            m = sqrtf(s);
            x = x0 / m; y = y0 / m; z = z0 / m;
            rx = 1.f / x; ry = 1.f / y; rz = 1.f / z;
        }
        const float l3 = fminf(fminf(fabsf(x), fabsf(y)), fabsf(z));
        const float sum = (fabsf(x) + fabsf(y)) + fabsf(z);
        slow = __builtin_amdgcn_ballot_w64(!(l3 >= 0x1p-60f && sum <= 0x1p60f));
    }
    return slow;
}

}  // namespace rtxd
