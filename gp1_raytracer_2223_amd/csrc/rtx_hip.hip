// rtx_hip.hip — MI355X (gfx950) render path behind the C-ABI of include/rtx.h.
//
// One HIP thread per pixel; one wave64 = an 8x8 pixel tile; one 256-thread workgroup =
// 16x16 pixels.  The BVH is traversed by the WAVE, not by the lane: a wave-uniform DFS
// stack of (node, 64-bit lane mask) lives in LDS, node/triangle/sphere/plane/light
// records are fetched once per wave through the scalar unit (s_load into SGPRs: the
// address is wave-uniform), and each lane evaluates its own ray against them under its
// mask bit.  A lane takes part in a node exactly when the reference's per-ray
// recursive DFS (source/Utils.h:246-288) would visit that node for its ray, in the same
// left-then-right order, so closest-hit tie-breaking (strict <) is the reference's.
// Shadow rays use the same packet traversal with __ballot early-out: a lane leaves the
// mask at its first occluder and the wave stops when every lane is occluded.
//
// Numerics: every float operation restates the reference in IEEE binary32 in the same
// order (built with -ffp-contract=off, correctly rounded div/sqrt); powf (Phong,
// Fresnel) is the device libm's and may differ from the host's by an ulp.
//
// This unit holds the render kernel and the launches that pick its instantiation (rtx_launch.h);
// the context, the upload, the frame and every policy are host units of their own.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "rtx.h"
#include "rtx_cull.h"
#include "rtx_fastdiv.h"
#include "rtx_kernels.h"
#include "rtx_variants.h"
#include "rtx_launch.h"

using namespace rtxd;

#if RTX_STAMPS
#define RTX_SPLIT_STAMP()                                                                          \
    if (lane == 0 && F.split_stamps) {                                                             \
        const unsigned long long d_ = __builtin_amdgcn_s_memrealtime() - t_start;                 \
        unsigned long long* x_ =                                                                   \
            F.split_stamps + 3 * (((PHASE - 1) * kMaxParts + part) * kStampShards + widx % kStampShards); \
        atomicAdd(x_, d_);                                                                         \
        atomicMax(x_ + 1, d_);                                                                     \
        atomicAdd(x_ + 2, static_cast<unsigned long long>(cnt.c[kWaveNodeTests] + cnt.c[kWaveTriTests])); \
    }
#else
#define RTX_SPLIT_STAMP()
#endif

// ====================================================================== device code
namespace {

__device__ __forceinline__ float smin(float a, float b) { return (b < a) ? b : a; }  // std::min
__device__ __forceinline__ float smax(float a, float b) { return (a < b) ? b : a; }  // std::max

__device__ __forceinline__ uint32_t uni(uint32_t x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ unsigned long long uni64(unsigned long long x) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(x));
    const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(x >> 32));
    return (static_cast<unsigned long long>(hi) << 32) | lo;
}
__device__ __forceinline__ unsigned long long ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }

// Scene records are immutable for a whole launch: they are read through the constant
// address space, so every wave-uniform read is an s_load through the scalar cache.  With
// generic pointers the backend needs a "no clobber" proof for s_load, which any
// side-effecting instruction on the path (s_memtime for the tile costs) defeats, and the
// reads silently become per-lane vector loads.
#define RTX_CONST __attribute__((address_space(4)))
typedef float cf4 __attribute__((ext_vector_type(4)));
typedef int ci4 __attribute__((ext_vector_type(4)));
typedef float cf16 __attribute__((ext_vector_type(16)));
__device__ __forceinline__ float4 ldc(const float4* base, uint32_t i) {
    const cf4 v = ((const RTX_CONST cf4*)base)[i];
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ int4 ldc(const int4* base, uint32_t i) {
    const ci4 v = ((const RTX_CONST ci4*)base)[i];
    return make_int4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ uint32_t ldc(const uint32_t* base, uint32_t i) {
    return ((const RTX_CONST uint32_t*)base)[i];
}
__device__ __forceinline__ float ldc(const float* base, uint32_t i) { return ((const RTX_CONST float*)base)[i]; }
typedef float cf8 __attribute__((ext_vector_type(8)));
// A wave-uniform value the optimiser cannot see through: a loop counter passed through it
// stays a 32-bit SGPR offset instead of being widened into a 64-bit pointer induction
// (which costs an s_add_u32/s_addc_u32 pair per record).
__device__ __forceinline__ uint32_t opaque(uint32_t x) {
    asm("" : "+s"(x));
    return x;
}
// Records at a BYTE offset: the offset goes into the SGPR-offset field of s_load, so a
// loop over records or a link walk costs no scalar address arithmetic.
__device__ __forceinline__ float4 ldcb16(const void* base, uint32_t off) {
    const cf4 v = *(const RTX_CONST cf4*)((const RTX_CONST char*)base + off);
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ int4 ldcb16i(const void* base, uint32_t off) {
    const ci4 v = *(const RTX_CONST ci4*)((const RTX_CONST char*)base + off);
    return make_int4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void ldcb32(const void* base, uint32_t off, float4& a, float4& b) {
    const cf8 v = *(const RTX_CONST cf8*)((const RTX_CONST char*)base + off);
    a = make_float4(v[0], v[1], v[2], v[3]);
    b = make_float4(v[4], v[5], v[6], v[7]);
}
// 64-byte record (Tri, NodePair): one s_load_dwordx16
__device__ __forceinline__ void ldcb64(const void* base, uint32_t off, float4& a, float4& b, float4& c, float4& d) {
    const cf16 v = *(const RTX_CONST cf16*)((const RTX_CONST char*)base + off);
    a = make_float4(v[0], v[1], v[2], v[3]);
    b = make_float4(v[4], v[5], v[6], v[7]);
    c = make_float4(v[8], v[9], v[10], v[11]);
    d = make_float4(v[12], v[13], v[14], v[15]);
}

struct Ray {
    float ox, oy, oz, dx, dy, dz, ix, iy, iz, tmin, tmax;
};

// dae::Ray constructor (DataTypes.h:549-564): inversedDir = 1 / dir.  `slow` = lanes whose
// direction is outside the fast reciprocal domain (rcp3_exact); every other lane has a
// finite, non-zero inverse direction — the FAST slab condition.
__device__ __forceinline__ Ray make_ray(float ox, float oy, float oz, float dx, float dy, float dz, float tmin,
                                        float tmax, unsigned long long& slow) {
    Ray r;
    r.ox = ox; r.oy = oy; r.oz = oz; r.dx = dx; r.dy = dy; r.dz = dz;
    slow = rcp3_exact(dx, dy, dz, r.ix, r.iy, r.iz);
    r.tmin = tmin; r.tmax = tmax;
    return r;
}
// ... for a direction whose inverse the caller already has (RTX_DIR_NORMALISE)
__device__ __forceinline__ Ray make_ray(float ox, float oy, float oz, float dx, float dy, float dz, float ix, float iy,
                                        float iz, float tmin, float tmax) {
    return {ox, oy, oz, dx, dy, dz, ix, iy, iz, tmin, tmax};
}

// HitTest_Sphere (Utils.h:52-66) in two steps, so that the square root (16 VALU when
// correctly rounded) runs only when some lane's ray passes within the radius:
//   sphere_perp: squared distance of the centre from the ray line (reject if r^2 < perp)
//   sphere_t:    t = proj - sqrt(r^2 - perp) and the [tmin, tmax] test
struct SphereProj {
    float proj, perp;
};
__device__ __forceinline__ SphereProj sphere_perp(const float4 s, const Ray& r) {
    const float ovx = s.x - r.ox, ovy = s.y - r.oy, ovz = s.z - r.oz;
    const float ovs = ovx * ovx + ovy * ovy + ovz * ovz;
    const float proj = r.dx * ovx + r.dy * ovy + r.dz * ovz;
    return {proj, ovs - proj * proj};
}
__device__ __forceinline__ float sphere_t(const float4 s, const SphereProj& q) { return q.proj - sqrtf(s.w - q.perp); }

// HitTest_Plane (Utils.h:84-97): t = num / den.  With tmin > 0 (every ray here), a hit
// needs t > 0, i.e. num and den non-zero with the same sign: RN(num/den) carries the exact
// sign of the quotient, 0/x, x/0 and NaN operands all fail t >= tmin.  `plane_cand`
// lets a wave skip the division when no lane can hit.
__device__ __forceinline__ float plane_num(const float4 p0, const float4 p1, const Ray& r) {
    return (p0.x - r.ox) * p1.x + (p0.y - r.oy) * p1.y + (p0.z - r.oz) * p1.z;
}
__device__ __forceinline__ float plane_den(const float4 p1, const Ray& r) {
    return r.dx * p1.x + r.dy * p1.y + r.dz * p1.z;
}
// The room's planes (kSpecRoomPlanes, rtx_kernels.h): plane k's normal is s = +-1 on axis
// A = kRoomAxes[k] and zero elsewhere, its origin finite with |p0| <= 2^64.  For a ray with a
// finite origin every other term of HitTest_Plane's two dot products is a signed zero (p0 - o
// cannot overflow), so the reference's num and den are s * a and s * d with
//   a = p0_A - o_A,   d = d_A
// whenever those are non-zero (x + +-0 = x, inf included), and its t = num / den = a / d (IEEE
// division is sign-symmetric); the same-sign and beyond tests of plane_cand read the same
// signs and magnitudes.  When a or d is zero the quotient is +-0, +-inf or NaN, which fails
// t >= tmin > 0 or t < tmax <= FLT_MAX in both forms whatever the zero's sign; so does a NaN /
// infinite direction component, which leaves d 0, +-inf or NaN here and den NaN in the
// reference (a normalised direction is finite unless its length was 0 or inf).  Same hits,
// same t, 1 VALU instead of 13 before the division.
template <int A>
__device__ __forceinline__ float room_a(const float4 p0, const Ray& r) {
    return A == 0 ? p0.x - r.ox : (A == 1 ? p0.y - r.oy : p0.z - r.oz);
}
template <int A>
__device__ __forceinline__ float room_d(const Ray& r) {
    return A == 0 ? r.dx : (A == 1 ? r.dy : r.dz);
}
template <int A>
__device__ __forceinline__ float room_inv(const Ray& r) {
    return A == 0 ? r.ix : (A == 1 ? r.iy : r.iz);
}
// f(integral_constant<int, k>) for the room's planes k = 0..4, in order
template <class Fn>
__device__ __forceinline__ void for_room_planes(Fn&& f) {
    f(std::integral_constant<int, 0>{});
    f(std::integral_constant<int, 1>{});
    f(std::integral_constant<int, 2>{});
    f(std::integral_constant<int, 3>{});
    f(std::integral_constant<int, 4>{});
}
__device__ __forceinline__ bool finite3(float x, float y, float z) {
    return __builtin_isfinite(x) & __builtin_isfinite(y) & __builtin_isfinite(z);
}
// Shadow rays (finite tmax): only lanes whose num and den have equal sign bits can hit
// (over-inclusive is harmless: it only decides whether the division runs; zeros and NaNs then
// fail the range test on t), and a lane whose exact |num| / |den| exceeds tmax cannot hit either —
// RN(num/den) >= tmax by monotonicity — and one fma tells it exactly: the sign of
// RN(|den| * tmax - |num|) is the sign of the exact value (an underflow to -0 reads as "not
// beyond", and a NaN or inf operand as well; the division then decides).  Walls behind the
// light are the common case, so most waves skip the division.
__device__ __forceinline__ unsigned long long plane_cand(float num, float den, float tmax) {
    const int same = (__float_as_int(num) ^ __float_as_int(den)) >= 0;
    const int beyond = fmaf(fabsf(den), tmax, -fabsf(num)) < 0.f;
    return ballot(same) & ballot(!beyond);   // (a ballot per compare: one of a conjunction goes through a VGPR boolean)
}

// HitTest_Triangle (Utils.h:109-184), Möller–Trumbore with the reference's cull rules
// (shadow rays swap front/back culling, :114-127).
//
// Written branch-free: every early `return false` of the reference becomes a term whose
// positive value means "reject", folded with v_max_f32 (which ignores NaN exactly as the
// reference's comparisons do: a NaN never rejects).  For binary32 x, y:
//   x < y  <=>  (y - x) > 0   (a non-zero exact difference never rounds to 0 or flips sign)
// so  |c| < EPS <=> EPS-|c| > 0,  u < 0 || u > 1 <=> max(-u, u-1) > 0,
//     v < 0 || (u+v) > 1 <=> max(-v, (u+v)-1) > 0,  t < tmin <=> tmin - t > 0.
// Cross products use the reduced form {a, -b, c}: identical to Vector3::Cross's
// UnitX*a - UnitY*b + UnitZ*c for finite inputs up to the sign of a zero, which none of
// the tests below can observe.  Returns the reject score; accept iff !(score > 0) && !(t >= tmax).
// `cs` is the mesh's cull sign: -1 FrontFaceCulling (reject cullDot < 0), +1
// BackFaceCulling (reject cullDot > 0), 0 NoCulling (the term 0*cullDot never exceeds 0);
// shadow rays pass -cs, which is the reference's front/back swap.
template <bool FAST>
__device__ __forceinline__ float tri_t(const float4 A, const float4 B, const float4 C, float cs, const Ray& r,
                                       float& t) {
    const float cullDot = A.w * r.dx + B.w * r.dy + C.w * r.dz;
    float rej = fmaxf(FLT_EPSILON - fabsf(cullDot), cs * cullDot);
    const float hx = r.dy * C.z - r.dz * C.y;
    const float hy = -(r.dx * C.z - r.dz * C.x);
    const float hz = r.dx * C.y - r.dy * C.x;
    const float a = B.x * hx + B.y * hy + B.z * hz;
    rej = fmaxf(rej, FLT_EPSILON - fabsf(a));
    // RN(1/a): lanes with |a| < EPS are rejected above whatever ai is, so only huge, inf
    // and NaN a need the IEEE sequence (NaN gives NaN either way).  FAST: every direction
    // is finite with |d| < 2 and the scene's |e1||e2| <= 2^56 (DevScene::tri_fast), so
    // |a| <= |e1||d||e2| < 2^60 and rcp_rn is exact without the check.
    float ai = rcp_rn(a);
    if (!FAST && __builtin_expect(fabsf(a) > 0x1p60f, 0)) ai = 1.f / a;
    const float sx = r.ox - A.x, sy = r.oy - A.y, sz = r.oz - A.z;
    const float u = ai * (sx * hx + sy * hy + sz * hz);
    rej = fmaxf(rej, fmaxf(-u, u - 1.f));
    const float qx = sy * B.z - sz * B.y;
    const float qy = -(sx * B.z - sz * B.x);
    const float qz = sx * B.y - sy * B.x;
    const float v = ai * (r.dx * qx + r.dy * qy + r.dz * qz);
    rej = fmaxf(rej, fmaxf(-v, (u + v) - 1.f));
    t = ai * (C.x * qx + C.y * qy + C.z * qz);
    return fmaxf(rej, r.tmin - t);
}

// Vector3::Cross (Vector3.cpp:50-54) as it is written, UnitX * a - UnitY * b + UnitZ * c: a term that
// is infinite or NaN reaches every component through its 0 * term.  The reduced form {a, -b, c} of
// tri_t equals it only while a, b and c are finite (up to the sign of a zero).
__device__ __forceinline__ void cross_ref(float ax, float ay, float az, float bx, float by, float bz, float& x,
                                          float& y, float& z) {
    const float a = ay * bz - az * by;
    const float b = ax * bz - az * bx;
    const float c = ax * by - ay * bx;
    x = (1.f * a - 0.f * b) + 0.f * c;
    y = (0.f * a - 1.f * b) + 0.f * c;
    z = (0.f * a - 0.f * b) + 1.f * c;
}

// tri_t with two wave-uniform early exits for the lanes in `act` (the ones whose result is
// used): after the cull test (Utils.h:114-127) and after the u range test (:160-163), the
// rest is skipped when no lane in `act` can still be accepted — the same early returns as
// the reference's, taken per wave.  Returns false (wave-uniform) when the triangle was
// skipped — no lane hits it — else true with the reject score in `rej_out` and t in `t`.
// (A uniform flag rather than a reject value: a phi of the reject compare is carried as a
// lane mask and rebuilt with v_cndmask + v_cmp per triangle.)
// CB (kSpecCullBack): the mesh culls back faces, so cs is +1 for camera rays and -1 for shadow
// rays (ANY) and cs * cullDot is +-cullDot exactly: a source negation instead of a multiply.
// XC (ray queries, rtx_query_kernel): both cross products as Vector3::Cross writes them (cross_ref),
// for rays outside the reduced form's domain.
template <bool FAST, bool CB = false, bool ANY = false, bool XC = false>
__device__ __forceinline__ bool tri_t_wave(const float4 A, const float4 B, const float4 C, float cs, const Ray& r,
                                           unsigned long long act, float& rej_out, float& t) {
    const float cullDot = A.w * r.dx + B.w * r.dy + C.w * r.dz;
    float rej = fmaxf(FLT_EPSILON - fabsf(cullDot), CB ? (ANY ? -cullDot : cullDot) : cs * cullDot);
    if ((ballot(!(rej > 0.f)) & act) == 0) return false;
    float hx, hy, hz;
    if constexpr (XC) {
        cross_ref(r.dx, r.dy, r.dz, C.x, C.y, C.z, hx, hy, hz);
    } else {
        hx = r.dy * C.z - r.dz * C.y;
        hy = -(r.dx * C.z - r.dz * C.x);
        hz = r.dx * C.y - r.dy * C.x;
    }
    const float a = B.x * hx + B.y * hy + B.z * hz;
    rej = fmaxf(rej, FLT_EPSILON - fabsf(a));
    float ai = rcp_rn(a);
    if (!FAST && __builtin_expect(fabsf(a) > 0x1p60f, 0)) ai = 1.f / a;
    const float sx = r.ox - A.x, sy = r.oy - A.y, sz = r.oz - A.z;
    const float u = ai * (sx * hx + sy * hy + sz * hz);
    rej = fmaxf(rej, fmaxf(-u, u - 1.f));
    if ((ballot(!(rej > 0.f)) & act) == 0) return false;
    float qx, qy, qz;
    if constexpr (XC) {
        cross_ref(sx, sy, sz, B.x, B.y, B.z, qx, qy, qz);
    } else {
        qx = sy * B.z - sz * B.y;
        qy = -(sx * B.z - sz * B.x);
        qz = sx * B.y - sy * B.x;
    }
    const float v = ai * (r.dx * qx + r.dy * qy + r.dz * qz);
    rej = fmaxf(rej, fmaxf(-v, (u + v) - 1.f));
    t = ai * (C.x * qx + C.y * qy + C.z * qz);
    rej_out = fmaxf(rej, r.tmin - t);
    return true;
}

// SlabTest_BVH (Utils.h:221-243).  FAST uses v_min/v_max_f32, which differ from std::min/
// std::max only when an operand is NaN; a NaN slab value needs (box - origin) * inv with
// an infinite inv component, so FAST is taken only when every live lane's inverse
// direction is finite (decided once per ray batch with a ballot).
// Returned as a wave lane mask: one v_cmp per condition straight into SGPRs (a ballot
// of the && would materialise the bool in a VGPR and compare it again).
// Node record (32 B): a = {min.x, max.x, min.y, max.y}, b = {min.z, max.z, link, ntri};
// link and triangle count are adjacent (one 64-bit SGPR pair).  (Packed f32 for the
// (min, max) pairs was measured 15-35 % slower: profiles/r01/ablate_history.md.)
// SLAB selects the formulation (all three give the reference's pass/fail bit):
//   kSlabExact  std::min/std::max restated (NaN-safe), any direction;
//   kSlabFast   v_min/v_max_f32, which differ from std::min/std::max only when an operand
//               is NaN; a NaN slab value needs (box - origin) * inv with an infinite inv
//               component, so it is taken only when every live lane's inverse direction is
//               finite (decided once per ray batch with a ballot);
//   kSlabOct    kSlabFast for a ray batch whose inverse directions have ONE sign per axis
//               (an octant), against the node copy ordered (near, far) for that octant:
//               the near and far planes are known, so min/max of each pair disappears.
// Returned as a wave lane mask: one v_cmp per condition straight into SGPRs (a ballot
// of the && would materialise the bool in a VGPR and compare it again).
enum { kSlabExact = 0, kSlabFast = 1, kSlabOct = 2 };
template <int SLAB>
__device__ __forceinline__ unsigned long long slab_mask(const float4 a, const float4 b, const Ray& r) {
    const float tx1 = (a.x - r.ox) * r.ix, tx2 = (a.y - r.ox) * r.ix;
    const float ty1 = (a.z - r.oy) * r.iy, ty2 = (a.w - r.oy) * r.iy;
    const float tz1 = (b.x - r.oz) * r.iz, tz2 = (b.y - r.oz) * r.iz;
    float tMin, tMax;
    if (SLAB == kSlabOct) {
        // Octant copy: per axis the record holds (near, far) = (lo, hi) where inv > 0 and
        // (hi, lo) where inv < 0, so rounding monotonicity gives t_near <= t_far per axis
        // (the pair's min and max); each value is the reference's own (same operands).
        tMin = fmaxf(fmaxf(fmaxf(tx1, ty1), tz1), 0x1p-149f);
        tMax = fminf(fminf(tx2, ty2), tz2);
        return ballot(tMax >= tMin);
    } else if (SLAB == kSlabFast) {
        tMin = fmaxf(fmaxf(fminf(tx1, tx2), fminf(ty1, ty2)), fminf(tz1, tz2));
        tMax = fminf(fminf(fmaxf(tx1, tx2), fmaxf(ty1, ty2)), fmaxf(tz1, tz2));
        // no NaN here: tMax > 0 && tMax >= tMin  <=>  tMax >= max(tMin, smallest denormal)
        // (f32 denormals are kept, .amdhsa_float_denorm_mode_32 = 3): one compare, no s_and
        return ballot(tMax >= fmaxf(tMin, 0x1p-149f));
    } else {
        tMin = smin(tx1, tx2);
        tMax = smax(tx1, tx2);
        tMin = smax(tMin, smin(ty1, ty2));
        tMax = smin(tMax, smax(ty1, ty2));
        tMin = smax(tMin, smin(tz1, tz2));
        tMax = smin(tMax, smax(tz1, tz2));
    }
    return ballot(tMax > 0) & ballot(tMax >= tMin);
}

// Exact cull (rtx_cull.h): a node the reference's slab test passes is skipped for
// a lane when no triangle below can pass HitTest_Triangle for its ray in a way that matters, so
// the visit would change nothing:
//   * the ray's LINE misses the node's tight box widened by the margin rtx_cull.h proves for the
//     ray's anchor (view camera / light): no triangle below can be accepted at all;
//   * closest hit: the line enters that box at n with n - dt > sc_t (dt: rtx_cull.h's bound on
//     |t~ - t*| for t~ <= the anchor's bt, valid while sc_t <= bt): every triangle below that
//     could be accepted has t~ > sc_t, so none replaces the scratch hit (strict <);
//   * shadow ray: n - dt > tmax or f + dt < tmin (f: where the line leaves the box): no accepted
//     t~ lies in [tmin, tmax).
// Record per node slot (same byte offset as the node): {c.x, c.y, c.z, E.x}, {E.y, E.z, dt, flag},
// box = c +- E (E includes the margin and the padding 16u (E + |c|) that covers this test's own
// rounding, so n is at most and f at least the exact entry and exit of the widened box; rounding
// of n - dt etc. is monotone, so each float comparison implies the exact one).  `k` = 16u |o| |inv|
// per axis covers the rounding of (c - o) * inv, or +inf for a lane outside the bound's domain
// (n = -inf, f = +inf: it passes every test).  Lanes of a FAST batch only (finite non-zero inverse
// directions, |inv| <= 2^64).  NaN-safe: max/min ignore a NaN operand (its axis is dropped) and a
// NaN comparison never culls.
struct CullRay {
    const float4* base;   // the anchor's records (null: no cull)
    float kx, ky, kz;
    float bt;             // the anchor's t bound for dt (closest hit: prune only while sc_t <= bt)
};
__device__ __forceinline__ void cull_nf(const float4 a, const float4 b, const Ray& r, const CullRay& q, float& n,
                                        float& f) {
    const float tx = (a.x - r.ox) * r.ix, ty = (a.y - r.oy) * r.iy, tz = (a.z - r.oz) * r.iz;
    const float hx = fmaf(a.w, fabsf(r.ix), q.kx), hy = fmaf(b.x, fabsf(r.iy), q.ky), hz = fmaf(b.y, fabsf(r.iz), q.kz);
    n = fmaxf(fmaxf(tx - hx, ty - hy), tz - hz);
    f = fminf(fminf(tx + hx, ty + hy), tz + hz);
}
// lanes that still have to enter the node whose record is (a, b); n: the entry (child ordering)
template <bool ANY>
__device__ __forceinline__ unsigned long long cull_pass(const float4 a, const float4 b, const Ray& r, const CullRay& q,
                                                        float sc_t, float& n) {
    float f;
    cull_nf(a, b, r, q, n, f);
    const float dt = b.z;
    bool keep = !(n > f);
    if (ANY) keep = keep & !(n - dt > r.tmax) & !(f + dt < r.tmin);
    else keep = keep & !((sc_t <= q.bt) & (n - dt > sc_t));
    return ballot(keep);
}
// 16u |o_k| |inv_k| per axis, or +inf (always pass) for a lane outside the bound's domain:
// |o_k| <= 2^40, |inv_k| <= 2^64 and `ok` (the caller's conditions on the direction and tmax)
__device__ __forceinline__ CullRay cull_ray(const float4* base, const Ray& r, bool ok, float bt) {
    CullRay q;
    q.base = base;
    q.bt = bt;
    ok = ok && fabsf(r.ox) <= 0x1p40f && fabsf(r.oy) <= 0x1p40f && fabsf(r.oz) <= 0x1p40f &&
         fabsf(r.ix) <= 0x1p64f && fabsf(r.iy) <= 0x1p64f && fabsf(r.iz) <= 0x1p64f;
    constexpr float k16u = 0x1p-20f;
    q.kx = ok ? (k16u * fabsf(r.ox)) * fabsf(r.ix) : INFINITY;
    q.ky = ok ? (k16u * fabsf(r.oy)) * fabsf(r.iy) : INFINITY;
    q.kz = ok ? (k16u * fabsf(r.oz)) * fabsf(r.iz) : INFINITY;
    return q;
}

// Octant of a FAST ray batch (every live inverse direction finite and non-zero): bit k set
// when axis k's inverse direction is negative for every lane in `mask` (non-empty), -1
// when the lanes disagree on some axis.  One code per lane from the sign bits, compared
// against the first masked lane's: a few VALU and one compare, no per-axis scalar logic.
__device__ __forceinline__ int batch_octant(const Ray& r, unsigned long long mask) {
    const uint32_t code = (__float_as_uint(r.ix) >> 31) | ((__float_as_uint(r.iy) >> 31) << 1) |
                          ((__float_as_uint(r.iz) >> 31) << 2);
    const uint32_t first = static_cast<uint32_t>(__builtin_ctzll(mask));
    const uint32_t c0 = __builtin_amdgcn_readlane(code, first);
    return (ballot(code == c0) & mask) == mask ? static_cast<int>(c0) : -1;
}
// The mesh record carries its cull sign as float bits (set at upload: -1 FrontFaceCulling,
// +1 BackFaceCulling, 0 NoCulling); shadow rays use the negation, the reference's swap.
__device__ __forceinline__ float cull_sign(int cs_bits, bool shadow) {
    const float cs = __int_as_float(cs_bits);
    return shadow ? -cs : cs;
}

struct alignas(64) NodePair {
    float4 l0, l1, r0, r1;   // left child (a, b) then right child (a, b), see slab_mask
};
// (link, ntri) of a child as one 64-bit value: link low, count high
__device__ __forceinline__ unsigned long long link_ntri(const float4 b) {
    return (static_cast<unsigned long long>(__float_as_uint(b.w)) << 32) | __float_as_uint(b.z);
}

struct Counts {
    uint32_t c[kNumCounters];
};

// Packet traversal of one mesh's BVH by the whole wave.
//
// A node is entered with the mask of lanes whose slab test on it passed; an inner node
// then tests BOTH children (adjacent, one 64-byte scalar load) for those lanes, descends
// into the left child and pushes the right one with its own pass mask.  Each lane thus
// evaluates exactly the slab tests and triangle tests of the reference's recursive DFS
// (Utils.h:246-288), triangles in the same left-to-right order.
//   closest (ANY = false): `sc_t` is the shared scratch HitRecord t of Scene.cpp:31 that
//       IntersectionTest_BVH compares against (Utils.h:270-273); t < sc_t replaces it.
//   any-hit (ANY = true, shadow rays, Scene::DoesHit): a lane leaves at its first
//       occluder; the wave leaves as soon as every lane in `mask` is occluded.
// COUNT: per-lane SURVEY §8(d) work counters, any-hit counted up to the first occluder.
// DFS below one node (link, ntri) that passed its slab test for the lanes in m.
template <bool ANY, bool FAST, bool COUNT>
__device__ void bvh_walk(const DevScene& S, float cs, const Ray& r, uint32_t link, uint32_t ntri, unsigned long long m,
                         unsigned long long mask, uint32_t lane, uint4* stk, unsigned long long* sT, float& sc_t,
                         uint32_t& sc_tri, unsigned long long& live, Counts& cnt, const uint32_t* occ_word = nullptr,
                         uint32_t occ_bit = 0) {
    int sp = 0;
    for (;;) {
        // invariant: the node (link, ntri) passed its slab test exactly for the lanes in m
        if (ntri) {
            if ((COUNT || RTX_STAMPS) && lane == 0) cnt.c[kWaveTriTests] += ntri;
            if (RTX_STAMPS && !COUNT && lane == 0) cnt.c[kTri] += ntri * __popcll(ANY ? (m & live) : m);
            const bool in = (m >> lane) & 1ull;
            for (uint32_t k = 0; k < ntri; ++k) {
                const uint32_t ti = link + k * 64u;   // byte offset of the triangle record
                Tri T;
                ldcb64(S.tris, ti, T.a, T.b, T.c, T.d);
                float t;
                const float rej = tri_t<FAST>(T.a, T.b, T.c, cs, r, t);
                if (ANY) {
                    if (COUNT && ((m & live) >> lane) & 1ull) cnt.c[kTri]++;
                    live &= ~(ballot(!(rej > 0.f)) & ballot(!(t >= r.tmax)) & m);
                } else {
                    if (COUNT && in) cnt.c[kTri]++;
                    const bool u = in & !(rej > 0.f) & !(t >= r.tmax) & (t < sc_t);
                    sc_t = u ? t : sc_t;
                    sc_tri = u ? ti : sc_tri;
                }
            }
            if (ANY && occ_word) {
                // split any-hit: drop the lanes another part has already found occluded
                const uint32_t o = __hip_atomic_load(occ_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                live &= ~ballot((o & occ_bit) != 0u);
            }
            if (ANY && (live & mask) == 0) return;
        } else {
            if ((COUNT || RTX_STAMPS) && lane == 0) cnt.c[kWaveNodeTests]++;
            if (RTX_STAMPS && !COUNT && lane == 0) cnt.c[kSlab] += 2 * __popcll(m);
            NodePair P;
            ldcb64(S.nodes, link, P.l0, P.l1, P.r0, P.r1);
            const unsigned long long ml = slab_mask<FAST ? kSlabFast : kSlabExact>(P.l0, P.l1, r) & m;
            const unsigned long long mr = slab_mask<FAST ? kSlabFast : kSlabExact>(P.r0, P.r1, r) & m;
            const bool in = COUNT && ((m >> lane) & 1ull);
            if (COUNT && in) cnt.c[kSlab]++;               // left child's test
            if (COUNT && !ANY && in) cnt.c[kSlab]++;       // right child's (closest: always reached)
            if (ml) {
                // an opaque copy keeps this test local to the block: a `mr != 0` shared with
                // the test below is hoisted and carried across blocks as a VGPR boolean
                // (s_cselect + v_cndmask + v_cmp per node pair)
                unsigned long long mrl = mr;
                asm("" : "+s"(mrl));
                if (mrl || (COUNT && ANY)) {               // any-hit COUNT: right is counted at pop
                    stk[sp] = make_uint4(__float_as_uint(P.r1.z), __float_as_uint(P.r1.w),
                                         static_cast<uint32_t>(mrl), static_cast<uint32_t>(mrl >> 32));
                    if (COUNT && ANY) sT[sp] = m;
                    ++sp;
                }
                link = __float_as_uint(P.l1.z);
                ntri = __float_as_uint(P.l1.w);
                m = ml;
                continue;
            }
            if (COUNT && ANY && in) cnt.c[kSlab]++;        // right child's test, reached now
            if (mr) {
                link = __float_as_uint(P.r1.z);
                ntri = __float_as_uint(P.r1.w);
                m = mr;
                continue;
            }
        }
        // pop the next pending right child
        for (;;) {
            if (sp == 0) return;
            --sp;
            const uint4 e = stk[sp];
            link = uni(e.x);
            ntri = uni(e.y);
            m = (static_cast<unsigned long long>(uni(e.w)) << 32) | uni(e.z);
            if (ANY) {
                if (COUNT) {
                    const unsigned long long tested = uni64(sT[sp]);
                    if (((tested & live) >> lane) & 1ull) cnt.c[kSlab]++;
                }
                m &= live;
            }
            if (m) break;
        }
    }
}

constexpr int kPlaneCache = 8;   // planes whose shadow-ray numerators are kept in LDS
// bvh_walk without counters, shaped for the scalar unit: one inner loop descends through
// inner nodes with scalar selects (no i1 value crosses a block, so nothing is carried as a
// VGPR boolean or a lane-mask flow variable), a dead end leaves it as an empty "leaf", and
// the pop loop is the only other path.  Same visits, tests and order as bvh_walk.
// `nb` is the node copy the slab form reads (the octant's (near, far) copy for kSlabOct).
// CULL: a child is entered only by the lanes cull_pass keeps, and the walk is ORDERED: the child
// most lanes enter first is walked first.  Shadow rays (RTX_CULL_ORDER_ANY): nearer occluders end
// their lanes sooner, and any-hit is a yes/no that no order changes.  Closest hit: the scratch hit
// is replaced by t < sc_t or, on a tie, by the lower triangle index — the reference's first-found winner whatever the visiting
// order, because left-then-right DFS order is increasing triangle index (the scene has the cull
// only when that holds, upload_scene; the split launches' key minimum rests on the same fact) — so
// nearer subtrees lower sc_t before farther ones are tested and cull_pass prunes those.
// COUNT (the counting variant of the culled walk, rtx_count_work_culled): per lane, the slab,
// exact-cull and triangle tests this walk executes for the lane (a lane in the node's mask is
// tested against both children), in `cp` — the executed work beside the reference's (bvh_walk).
// XC (ray queries): the triangle test outside its fast domains — Vector3::Cross as written
// (cross_ref) and the |a| > 2^60 check of tri_t<false> — whatever the slab form.
template <bool ANY, int SLAB, bool CB = false, bool CULL = false, bool COUNT = false, bool XC = false>
__device__ void bvh_walk_lean(const DevScene& S, const float4* nb, float cs, const Ray& r, uint32_t link,
                              uint32_t ntri, unsigned long long m, unsigned long long mask, uint32_t lane, uint4* stk,
                              float& sc_t, uint32_t& sc_tri, unsigned long long& live, const uint32_t* occ_word,
                              uint32_t occ_bit, const CullRay& cq = CullRay{}, Counts* cp = nullptr) {
    constexpr bool FAST = SLAB != kSlabExact;
    constexpr bool ORD = CULL && (!ANY || RTX_CULL_ORDER_ANY);
    uint32_t sp = 0;
    for (;;) {
        while (ntri == 0) {
            NodePair P;
            ldcb64(nb, link, P.l0, P.l1, P.r0, P.r1);
            // the pair's cull records at the same offset, loaded beside the pair (one memory
            // latency per step, not two: the shadow walk had issued it only after the slab tests)
            [[maybe_unused]] NodePair Q;
            if (CULL) ldcb64(cq.base, link, Q.l0, Q.l1, Q.r0, Q.r1);
            if constexpr (COUNT) {
                if ((m >> lane) & 1ull) cp->c[kSlab] += 2;
                if (lane == 0) cp->c[kWaveNodeTests]++;
            }
            unsigned long long ml = slab_mask<SLAB>(P.l0, P.l1, r) & m;
            unsigned long long mr = slab_mask<SLAB>(P.r0, P.r1, r) & m;
            [[maybe_unused]] bool rfirst = false;
            if (CULL) {
                // only pairs whose records are flagged worth testing (cull_write), and only when
                // some lane entered a child
                if ((__float_as_uint(Q.l1.w) | __float_as_uint(Q.r1.w)) && (ml | mr)) {
                    if constexpr (COUNT) {
                        if ((m >> lane) & 1ull) cp->c[kCullTests] += 2;
                    }
                    float nl, nr;
                    ml &= cull_pass<ANY>(Q.l0, Q.l1, r, cq, sc_t, nl);
                    mr &= cull_pass<ANY>(Q.r0, Q.r1, r, cq, sc_t, nr);
                    if (ORD) {   // right first when most lanes that enter both enter it first
                        const unsigned long long both_m = ml & mr;
                        rfirst = 2 * __popcll(ballot(nr < nl) & both_m) > __popcll(both_m);
                    }
                }
            }
            if (ORD && rfirst) {   // walk the right child first: swap the pair's roles
                const unsigned long long t0 = ml;
                ml = mr;
                mr = t0;
                const float4 t1 = P.l1;
                P.l1 = P.r1;
                P.r1 = t1;
            }
            // next (link, ntri): left, else right, else a dead end taken as an empty leaf
            // (ntri = 1 with m = 0); `both` = mr if the left child is taken too (the right
            // one then waits on the stack).  Written as 64-bit s_cselects on one SCC each:
            // the compiler materialises every `x != 0` as a -1/0 SGPR pair and ANDs them.
            unsigned long long nx, both;
            asm("s_cmp_lg_u64 %[mr], 0\n\t"
                "s_cselect_b64 %[nx], %[lr], %[dead]\n\t"
                "s_cmp_lg_u64 %[ml], 0\n\t"
                "s_cselect_b64 %[nx], %[ll], %[nx]\n\t"
                "s_cselect_b64 %[both], %[mr], 0\n\t"
                "s_cselect_b64 %[m], %[ml], %[mr]"
                : [nx] "=&s"(nx), [both] "=&s"(both), [m] "=&s"(m)
                : [mr] "s"(mr), [ml] "s"(ml), [lr] "s"(link_ntri(P.r1)), [ll] "s"(link_ntri(P.l1)),
                  [dead] "s"(1ull << 32)
                : "scc");
            if (both) {
                stk[sp] = make_uint4(__float_as_uint(P.r1.z), __float_as_uint(P.r1.w), static_cast<uint32_t>(mr),
                                     static_cast<uint32_t>(mr >> 32));
                ++sp;
            }
            link = static_cast<uint32_t>(nx);
            // opaque: a 32-bit s_cmp for the loop test (else it becomes a 64-bit v_cmp on nx)
            ntri = opaque(static_cast<uint32_t>(nx >> 32));
        }
        if (m) {
            const bool in = (m >> lane) & 1ull;
            // split any-hit: the other parts' occlusion bits, read before the leaf's tests so the
            // L2 round trip overlaps them (RTX_OCC_POLL, rtx_variants.h)
            uint32_t occ_pre = 0u;
            if (ANY && RTX_OCC_POLL == 2 && occ_word)
                occ_pre = __hip_atomic_load(occ_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            for (uint32_t k = 0; k < ntri; ++k) {
                const uint32_t ti = link + k * 64u;
                Tri T;
                ldcb64(S.tris, ti, T.a, T.b, T.c, T.d);
                if constexpr (COUNT) {
                    if (((ANY ? (m & live) : m) >> lane) & 1ull) cp->c[kTri]++;
                    if (lane == 0) cp->c[kWaveTriTests]++;
                }
                float t;
                float rej;
                if (!tri_t_wave<FAST && !XC, CB, ANY, XC>(T.a, T.b, T.c, cs, r, ANY ? (m & live) : m, rej, t)) continue;
                if (ANY) {
                    live &= ~(ballot(!(rej > 0.f)) & ballot(!(t >= r.tmax)) & m);
                } else {
                    const bool better = CULL ? ((t < sc_t) | ((t == sc_t) & (ti < sc_tri))) : (t < sc_t);
                    const bool u = in & !(rej > 0.f) & !(t >= r.tmax) & better;
                    sc_t = u ? t : sc_t;
                    sc_tri = u ? ti : sc_tri;
                }
            }
            if (ANY && RTX_OCC_POLL != 0 && occ_word) {
                const uint32_t o = RTX_OCC_POLL == 2
                                       ? occ_pre
                                       : __hip_atomic_load(occ_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                live &= ~ballot((o & occ_bit) != 0u);
            }
            if (ANY && (live & mask) == 0) return;
        }
        for (;;) {
            if (sp == 0) return;
            --sp;
            const uint4 e = stk[sp];
            link = uni(e.x);
            ntri = uni(e.y);
            m = (static_cast<unsigned long long>(uni(e.w)) << 32) | uni(e.z);
            if (ANY) m &= live;
            if (m) break;
        }
    }
}

// SLAB = kSlabOct: `oct` is the batch's octant (batch_octant), else ignored.
// CULL (SLAB != kSlabExact, !COUNT): the exact cull of the anchor `cq` (cull_mask) beside every
// slab test, the root's included.
// XC: bvh_walk_lean's (ray queries; never with COUNT).
template <bool ANY, int SLAB, bool COUNT, bool CB = false, bool CULL = false, bool XC = false>
__device__ void mesh_traverse(const DevScene& S, const int4 M, const Ray& r, int oct, unsigned long long mask,
                              uint32_t lane, uint4* stk, unsigned long long* sT, float& sc_t, uint32_t& sc_tri,
                              unsigned long long& live, Counts& cnt, const CullRay& cq = CullRay{}) {
    static_assert(!CULL || SLAB != kSlabExact, "the cull runs in FAST batches of the lean walk only");
    static_assert(!XC || (!COUNT && !RTX_STAMPS_WALK), "the reference's cross products are the lean walk's only");
    constexpr bool FAST = SLAB != kSlabExact;
    if (M.y == 0) return;
    const bool OCT = SLAB == kSlabOct && !COUNT && !RTX_STAMPS_WALK;
    const float4* nb = OCT ? reinterpret_cast<const float4*>(reinterpret_cast<const char*>(S.nodes) +
                                                             static_cast<uint32_t>(oct) * S.oct_bytes)
                           : S.nodes;
    // root (odd global index; every child pair starts at an even one, 64-B aligned)
    float4 b0, b1;
    ldcb32(nb, static_cast<uint32_t>(M.x), b0, b1);   // M.x: the root's byte offset
    [[maybe_unused]] float4 c0, c1;   // the root's cull record, loaded beside it
    if (CULL) ldcb32(cq.base, static_cast<uint32_t>(M.x), c0, c1);
    if (COUNT && ((mask >> lane) & 1ull)) cnt.c[kSlab]++;
    unsigned long long m =
        (OCT ? slab_mask<kSlabOct>(b0, b1, r) : slab_mask<FAST ? kSlabFast : kSlabExact>(b0, b1, r)) & mask;
    if (CULL && m) {
        float n;
        if (__float_as_uint(c1.w)) {
            if (COUNT && ((m >> lane) & 1ull)) cnt.c[kCullTests]++;
            m &= cull_pass<ANY>(c0, c1, r, cq, sc_t, n);
        }
    }
    if (m == 0) return;
    // The exact walk is where every ray outside the reduced cross products' domain ends up (a slow lane, a
    // scene that is not tri_fast), a frame's as well as a query's: it takes Vector3::Cross as written.
    constexpr bool XCE = XC || (SLAB == kSlabExact && !COUNT && !RTX_STAMPS_WALK);
    if ((!COUNT || CULL) && !RTX_STAMPS_WALK)
        bvh_walk_lean<ANY, OCT ? kSlabOct : (FAST ? kSlabFast : kSlabExact), CB, CULL, COUNT, XCE>(
            S, nb, cull_sign(M.z, ANY), r, __float_as_uint(b1.z), __float_as_uint(b1.w), m, mask, lane, stk, sc_t,
            sc_tri, live, nullptr, 0u, cq, &cnt);
    else
        bvh_walk<ANY, FAST, COUNT>(S, cull_sign(M.z, ANY), r, __float_as_uint(b1.z), __float_as_uint(b1.w), m, mask,
                                   lane, stk, sT, sc_t, sc_tri, live, cnt);
}

// One part of a split traversal: the lanes that reach frontier node E (slab tests of the
// root and of every node on E's path, exactly the tests the full DFS makes on the way
// down), then the DFS of E's subtree.  Parts partition the triangles, so the closest-hit
// result is the minimum of the parts' (t, triangle index) keys — left-then-right DFS
// order is increasing triangle index (checked at upload), which makes the key minimum
// the reference's first-found, strict-< winner — and occlusion is the OR of the parts.
// SLAB = kSlabOct: `oct` is the batch's octant (batch_octant) and the part walks that copy.
// CB: kSpecCullBack (tri_t_wave).
// CULL: as mesh_traverse, on the part's path and below it.
// Returns, when `timed` (motion mode, FrameArgs::part_cost), the duration of the walk below E in
// cycles (0 when no lane reaches E): the part's share of the tile's one-piece cost; else 0.
template <bool ANY, int SLAB, bool CB = false, bool CULL = false>
__device__ unsigned long long part_traverse(const DevScene& S, const int4 E, const Ray& r, int oct,
                                            unsigned long long mask, uint32_t lane, uint4* stk, float& sc_t,
                                            uint32_t& sc_tri, unsigned long long& live, Counts& cnt,
                                            const uint32_t* occ_word = nullptr, uint32_t occ_bit = 0,
                                            const CullRay& cq = CullRay{}, bool timed = false) {
    static_assert(!CULL || SLAB != kSlabExact, "the cull runs in FAST batches only");
    constexpr bool FAST = SLAB != kSlabExact;
    if (E.x < 0) return 0;   // unused entry of a device-animated mesh's reserved frontier
    const int4 M = ldcb16i(S.meshes, static_cast<uint32_t>(E.x) * 16u);
    const float4* nb = SLAB == kSlabOct ? reinterpret_cast<const float4*>(reinterpret_cast<const char*>(S.nodes) +
                                                                          static_cast<uint32_t>(oct) * S.oct_bytes)
                                        : S.nodes;
    float4 b0, b1;
    ldcb32(nb, static_cast<uint32_t>(M.x), b0, b1);   // M.x: the root's byte offset
    [[maybe_unused]] float4 q0, q1;   // cull records loaded beside their nodes (one latency per step)
    if (CULL) ldcb32(cq.base, static_cast<uint32_t>(M.x), q0, q1);
    unsigned long long m = slab_mask<SLAB>(b0, b1, r) & mask;
    if (CULL && m) {
        float n;
        if (__float_as_uint(q1.w)) m &= cull_pass<ANY>(q0, q1, r, cq, sc_t, n);
    }
    uint32_t link = __float_as_uint(b1.z), ntri = __float_as_uint(b1.w);
    const uint32_t path = static_cast<uint32_t>(E.z);
    for (int d = 0; d < E.w && m; ++d) {
        NodePair P;
        ldcb64(nb, link, P.l0, P.l1, P.r0, P.r1);
        const bool right = (path >> d) & 1u;
        if (CULL) ldcb32(cq.base, link + (right ? 32u : 0u), q0, q1);
        const float4 c0 = right ? P.r0 : P.l0, c1 = right ? P.r1 : P.l1;
        m &= slab_mask<SLAB>(c0, c1, r);
        if (CULL) {
            float n;
            if (__float_as_uint(q1.w)) m &= cull_pass<ANY>(q0, q1, r, cq, sc_t, n);
        }
        link = __float_as_uint(c1.z);
        ntri = __float_as_uint(c1.w);
    }
    if (m == 0) return 0;
    // (read unconditionally: a `timed` test here made the compiler version the walk loop)
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    if (!RTX_STAMPS_WALK)
        bvh_walk_lean<ANY, SLAB, CB, CULL, false, SLAB == kSlabExact>(S, nb, cull_sign(M.z, ANY), r, link, ntri, m, mask,
                                                                      lane, stk, sc_t, sc_tri, live, occ_word, occ_bit,
                                                                      cq);   // (the exact walk: cross products as written)
    else
        bvh_walk<ANY, FAST, false>(S, cull_sign(M.z, ANY), r, link, ntri, m, mask, lane, stk, nullptr, sc_t, sc_tri,
                                   live, cnt, occ_word, occ_bit);
    return timed ? __builtin_amdgcn_s_memtime() - t0 : 0ull;   // (timed: the caller's use only)
}

struct RGB {
    float r, g, b;
};

// Material::Shade (Material.h:41-123) via BRDFs.h; m2.yzw holds (rgb*kd)/PI computed on
// the host with the same binary32 operations (BRDF::Lambert, BRDFs.h:14-17).
// KINDS: the material kinds the scene's geometry can hit (kSpecKind* bits, established by the
// host at upload; 0 = any).  Only their branches are compiled; a Lambert-only scene's BRDF is
// the precomputed constant with no dispatch at all.
template <int KINDS = 0>
__device__ __forceinline__ RGB shade(const DevScene& S, uint32_t mi, float nx, float ny, float nz, float lx, float ly,
                                     float lz, float vx, float vy, float vz, Counts& cnt, bool count) {
    constexpr int K = KINDS ? KINDS : kSpecKindAll;
    if (K == kSpecKindLambert) {
        const float4 m2 = ldc(S.materials, 3 * mi + 2);
        if (count) cnt.c[kShadeLambert]++;
        return {m2.y, m2.z, m2.w};
    }
    const float4 m0 = ldc(S.materials, 3 * mi), m1 = ldc(S.materials, 3 * mi + 1), m2 = ldc(S.materials, 3 * mi + 2);
    const int kind = __float_as_int(m0.x);
    RGB c{0.f, 0.f, 0.f};
    if ((K & kSpecKindSolid) && kind == RTX_MAT_SOLID_COLOR) {
        c = {m0.y, m0.z, m0.w};
    } else if ((K & kSpecKindLambert) && kind == RTX_MAT_LAMBERT) {
        if (count) cnt.c[kShadeLambert]++;
        c = {m2.y, m2.z, m2.w};
    } else if ((K & kSpecKindPhong) && kind == RTX_MAT_LAMBERT_PHONG) {
        if (count) { cnt.c[kShadeLambert]++; cnt.c[kShadePhong]++; }
        // BRDF::Phong (BRDFs.h:33-40)
        const float s2 = 2.f * smax(nx * lx + ny * ly + nz * lz, 0.f);
        const float rx = lx - nx * s2, ry = ly - ny * s2, rz = lz - nz * s2;
        const float cosa = smax(rx * vx + ry * vy + rz * vz, 0.f);
        const float spec = m1.y * powf(cosa, m1.z);
        c = {m2.y + spec, m2.z + spec, m2.w + spec};
    } else if ((K & kSpecKindCT) && kind == RTX_MAT_COOK_TORRANCE) {
        if (count) cnt.c[kShadeCT]++;
        float hx = vx + lx, hy = vy + ly, hz = vz + lz;
        const float hm = sqrtf(hx * hx + hy * hy + hz * hz);
        hx = hx / hm; hy = hy / hm; hz = hz / hm;
        const bool dielectric = (m1.w == 0.f);
        const float f0r = dielectric ? 0.04f : m0.y, f0g = dielectric ? 0.04f : m0.z, f0b = dielectric ? 0.04f : m0.w;
        const float p = powf(1.f - smax(hx * vx + hy * vy + hz * vz, 0.f), 5.f);
        const float Fr = f0r + ((1.f - f0r) * p), Fg = f0g + ((1.f - f0g) * p), Fb = f0b + ((1.f - f0b) * p);
        const float rough = m2.x;
        const float a = rough * rough;
        const float sqrA = a * a;
        const float ndh = smax(nx * hx + ny * hy + nz * hz, 0.f);
        const float in = (ndh * ndh) * ((a * a) - 1.f) + 1.f;
        const float D = sqrA / (RTX_PI * (in * in));
        const float k = ((a + 1.f) * (a + 1.f)) / 8.f;
        const float cv = smax(nx * vx + ny * vy + nz * vz, 0.f);
        const float cl = smax(nx * lx + ny * ly + nz * lz, 0.f);
        const float G = (cv / ((cv * (1.f - k)) + k)) * (cl / ((cl * (1.f - k)) + k));
        const float den = (4.f * smax(vx * nx + vy * ny + vz * nz, 0.0001f)) * smax(lx * nx + ly * ny + lz * nz, 0.0001f);
        const float kr = dielectric ? 1.f - Fr : 0.f, kg = dielectric ? 1.f - Fg : 0.f, kb = dielectric ? 1.f - Fb : 0.f;
        c.r = (m0.y * kr) / RTX_PI + ((Fr * D) * G) / den;
        c.g = (m0.z * kg) / RTX_PI + ((Fg * D) * G) / den;
        c.b = (m0.w * kb) / RTX_PI + ((Fb * D) * G) / den;
    }
    return c;
}

// motion mode (FrameArgs::part_cost): a split launch's wave adds the duration of its walk below
// its frontier part (cycles) to its tile's cost, in the tile cost's unit (16 cycles).  The parts'
// walks partition the one-piece walk, so their sum stands for the tile's one-piece cost without
// each part wave's fixed work (ray, planes, the part's path), which would keep a tile that stopped
// being heavy in the split set.
__device__ __forceinline__ void part_cost_add(uint32_t* cost, unsigned long long dt) {
    dt >>= 4;
    atomicAdd(cost, static_cast<uint32_t>(dt < 0xffffffffull ? dt : 0xffffffffull));
}

__device__ __forceinline__ uint32_t q8(float c) {
    // static_cast<uint8_t>(c * 255) as x86 compiles it: cvttss2si then the low byte
    // (NaN and out-of-int32-range values give 0x80000000 -> 0).
    const float x = c * 255;
    if (!(x > -2147483648.f && x < 2147483648.f)) return 0u;
    return static_cast<uint32_t>(static_cast<int32_t>(x)) & 0xffu;
}

}  // namespace

// Renderer::RenderPixel (source/Renderer.cpp:100-182) for a 16x16 tile per workgroup.
//
// PHASE 0 renders every tile except the heavy ones.  A heavy tile (measured cost far above
// the frame's per-slot share, see rtx_reorder_kernel) is rendered by three launches over the
// BVH frontier parts instead, so its serial traversal work is spread over many workgroups:
//   PHASE 1  grid (heavy, parts):          closest hit of one part -> atomicMin of the
//                                          {t bits, triangle} key per pixel
//   PHASE 2  grid (heavy, parts, lights):  shadow ray of one light against one part ->
//                                          atomicOr of the light's occlusion bit
//   PHASE 3  grid (heavy):                 hit record from the key, spheres/planes
//                                          occlusion + the bits, shading, output
// A light-major frame (FrameArgs::lm_*, small launches: a stripe share) replaces PHASE 0 by
//   PHASE 4  grid (tiles):                 PHASE 0 up to the hit record, which it writes
//   PHASE 5  persistent waves over the (tile, light) items: that light's shadow ray from the
//                                          record -> the occluded lanes; the tile's last light wave
//                                          shades every light in order (the occlusion published)
// The hit pass (rtx_render_aov*, FrameArgs::aov_*) is a launch of its own:
//   PHASE 7  grid (tiles):                 PHASE 0 up to the hit record, whose t, normal, material and
//                                          primitive it writes into the requested planes; no light loop
// Deferred shading (rtx_shade_aov*) is the other half, also one launch:
//   PHASE 8  grid (tiles):                 the hit record read from a stored hit pass's four planes (no
//                                          closest-hit work), then PHASE 0 from originOffset on
// The shadow pass (rtx_render_shadows_async) is PHASE 8 up to the occlusion decision:
//   PHASE 9  grid (tiles):                 the hit record from the planes, every light's shadow ray by the
//                                          walk PHASE 8 takes; bit l of the pixel's word (FrameArgs::occ_bits,
//                                          here the shadow plane, frame layout) = light l is occluded
// (rtx_relight_kernel, below, shades the planes plus that word without a ray.)
// Every phase recomputes the primary ray and the sphere/plane hits with the same code, so
// all of them see bit-identical values.
// DEEP: the variant for scenes whose BVH is kStackDepth or more levels deep (a DFS stack of
// kStackDepthDeep entries per wave in LDS; fewer waves fit a CU, so it is used only then).
// HSTK (with DEEP): the stacks in HBM instead (DevScene::hstk, any depth: the reference's
// recursion has no limit), for trees kStackDepthDeep or more levels deep.
// SPEC (kSpec* bits, rtx_kernels.h): uniform facts of the scene and frame the host checked at
// launch, compiled in instead of branched on (same operations, so the same pixels; fewer
// uniform branches, selects and registers; constant plane / mesh counts unroll their loops:
// Bunny 74.2 -> 61.2 us with RTX_SPEC_WAVES).
// Occupancy targets of the specialised kernels.  The variants with a constant mesh count ask for
// 8 waves per SIMD: the Lambert-only one then needs 47 VGPRs and 78 SGPRs (8 spilled to VGPR
// lanes, outside the loops), so the SGPR file no longer caps it at 7 waves like the generic
// kernel's 106 SGPRs (Bunny 61.1 -> 60.6 us, Bunny + 8 lights 427 -> 418 us; 10 waves: no gain);
// W4_Optional's variant 231 -> 223 us.  The variant with spheres and meshes stays at 7 (8: +4 %).
// CULLK: the variant with the exact cull (DevScene::cull; launched only for scenes that have the
// records — the code of the cull paths costs the kernel without them registers and 8 %).
// SS: the variant of a supersampled frame (FrameArgs::ss_log2 > 0) for the phases with the output
// epilogue (0, 3, 6): the frame is the sample frame and the epilogue resolves each pixel's k x k
// samples across the wave.  A variant of its own so that the plain kernels stay the code they were
// (as a run-time branch it moved their VGPR counts by 1-2: profiles/ss/resource_usage.txt).
// The pieces of Renderer::RenderPixel that render_tile and rtx_relight_kernel (below) both run, each stated
// once and expanded in both, so the relight's arithmetic is the frame's by construction.  Macros, not
// functions: as __forceinline__ functions they left the values alone but moved the register allocation of
// 128 of the render kernel's 162 instantiations (tools/codeobj_diff.py), and as macros render_tile is the
// text it was.  They name the variables of the scope they expand in.
// RTX_DIR_NORMALISE: the magnitude M of the direction X, Y, Z, the direction normalised by it, and the ray
// constructor's inverse direction IX, IY, IZ with its slow ballot SLOW (make_ray) for the expansions that cast
// the ray; the others leave them unused.
#define RTX_DIR_NORMALISE(ONE, X, Y, Z, M, IX, IY, IZ, SLOW)                                      \
    float M, IX, IY, IZ;                                                                          \
    const unsigned long long SLOW = norm_ray3<ONE>(X, Y, Z, M, IX, IY, IZ);                       \
    (void)IX; (void)IY; (void)IZ; (void)SLOW
// RTX_PRIMARY_DIR: the primary ray's direction dx, dy, dz, normalised from the magnitude dm
// (Renderer.cpp:104-114; Matrix::TransformVector Matrix.cpp:35-42).
// (px + 0.5f) / W and (2 * (py + 0.5f)) / H as Markstein quotients with the exact
// reciprocals RN(1/W), RN(1/H) (divided on the host, FrameArgs): numerators in [0.5, 2^17], divisors in
// [1, 2^16] lie inside div_rn's domain (rtx_fastdiv.h), so each is the IEEE quotient.
#define RTX_PRIMARY_DIR(F, V, ONE)                                                                \
    const int W = static_cast<int>(F.width), H = static_cast<int>(F.height);                      \
    const float fW = static_cast<float>(W), fH = static_cast<float>(H);                           \
    const float cx = (2.f * div_rn(px + 0.5f, fW, F.inv_width) - 1) * F.aspect * V.fov;           \
    const float cy = (1.f - div_rn(2.f * (py + 0.5f), fH, F.inv_height)) * V.fov;                 \
    float dx = V.right[0] * cx + V.up[0] * cy + V.forward[0] * 1.f;                               \
    float dy = V.right[1] * cx + V.up[1] * cy + V.forward[1] * 1.f;                               \
    float dz = V.right[2] * cx + V.up[2] * cy + V.forward[2] * 1.f;                               \
    RTX_DIR_NORMALISE(ONE, dx, dy, dz, dm, dix, diy, diz, dslow) /* dx /= dm; ... (Vector3::Normalize) */
// RTX_LIGHT_DIR: LightUtils::GetDirectionToLight (Utils.h:341-353) from originOffset: lx, ly, lz normalised
// from the magnitude mag (the shadow ray's tmax), for the light record L0 of type ltype.
#define RTX_LIGHT_DIR(ONE)                                                                        \
    const bool known = (ltype == RTX_LIGHT_POINT || ltype == RTX_LIGHT_DIRECTIONAL);              \
    float lx = known ? L0.x - oox : 0.f, ly = known ? L0.y - ooy : 0.f, lz = known ? L0.z - ooz : 0.f; \
    RTX_DIR_NORMALISE(ONE, lx, ly, lz, mag, lix, liy, liz, lslow)
// RTX_LIGHT_TERM: one unoccluded light's term of lighting mode MODE (Renderer.cpp:143-175) added to fr, fg,
// fb; KINDS and COUNT are shade's.
#define RTX_LIGHT_TERM(MODE, KINDS, COUNT)                                                        \
    if (MODE == RTX_MODE_COMBINED || MODE == RTX_MODE_RADIANCE) {                                 \
        /* LightUtils::GetRadiance (Utils.h:355-369) at hit.origin */                             \
        float s = 0.f;                                                                            \
        bool any = true;                                                                          \
        if (ltype == RTX_LIGHT_POINT) {                                                           \
            const float ex = L0.x - hx, ey = L0.y - hy, ez = L0.z - hz;                           \
            s = L1.w / (ex * ex + ey * ey + ez * ez);                                             \
        } else if (ltype == RTX_LIGHT_DIRECTIONAL) {                                              \
            s = L1.w;                                                                             \
        } else {                                                                                  \
            any = false;                                                                          \
        }                                                                                         \
        const float rr = any ? L1.x * s : 0.f, rg = any ? L1.y * s : 0.f, rb = any ? L1.z * s : 0.f; \
        if (MODE == RTX_MODE_RADIANCE) {                                                          \
            fr += rr; fg += rg; fb += rb;                                                         \
        } else {                                                                                  \
            const float oa = smax(nx * lx + ny * ly + nz * lz, 0.f);                              \
            const RGB br = shade<KINDS>(S, mat, nx, ny, nz, lx, ly, lz, vx, vy, vz, cnt, COUNT);  \
            fr += (rr * oa) * br.r; fg += (rg * oa) * br.g; fb += (rb * oa) * br.b;               \
        }                                                                                         \
    } else if (MODE == RTX_MODE_OBSERVED_AREA) {                                                  \
        const float oa = smax(nx * lx + ny * ly + nz * lz, 0.f);                                  \
        fr += oa; fg += oa; fb += oa;                                                             \
    } else if (MODE == RTX_MODE_BRDF) {                                                           \
        const RGB br = shade<KINDS>(S, mat, nx, ny, nz, lx, ly, lz, vx, vy, vz, cnt, COUNT);      \
        fr += br.r; fg += br.g; fb += br.b;                                                       \
    }
// RTX_MAX_TO_ONE: ColorRGB::MaxToOne (ColorRGB.h:12-17) on fr, fg, fb.  RTX_PACK_PX: their frame-buffer word
// in F's pixel format.
#define RTX_MAX_TO_ONE()                                                                          \
    const float mv = smax(fr, smax(fg, fb));                                                      \
    if (mv > 1.f) { fr /= mv; fg /= mv; fb /= mv; }
#define RTX_PACK_PX(F) ((q8(fr) << F.rshift) | (q8(fg) << F.gshift) | (q8(fb) << F.bshift) | F.amask)
#define f_mode (kComb ? RTX_MODE_COMBINED : F.mode)
#define f_shadows (kComb ? 1 : F.shadows)
#define n_sph (kNoSph ? 0u : S.n_spheres)
#define n_pl (kP5 ? 5u : S.n_planes)          // constant trip counts: the plane and mesh loops unroll
#define n_mesh (kNoMesh ? 0u : (kOneMesh ? 1u : S.n_meshes))
// One wave tile of one phase (rtx_render_kernel below dispatches the tiles and describes the phases): `widx` = the
// wave's index in the launch (PHASE 5: its item), `stk` / `sT` its DFS stacks, `pnum` its shadow-ray
// plane numerators in LDS.
// A split wave's duration for the frontier refinement (FrameArgs::part_max), sharded by wave.
template <int PHASE>
__device__ __forceinline__ void part_stat(const FrameArgs& F, uint32_t part, uint32_t widx, uint32_t lane,
                                          unsigned long long t0) {
    if (!F.part_max || lane != 0) return;
    const unsigned long long d = (__builtin_amdgcn_s_memtime() - t0) >> 4;
    atomicMax(F.part_max + ((static_cast<uint32_t>(PHASE) - 1u) * kMaxParts + part) * kPartShards + widx % kPartShards,
              static_cast<uint32_t>(d < 0xffffffffull ? d : 0xffffffffull));
}

// Supersampling resolve (FrameArgs::ss_log2): v + the value of lane ^ X, in every lane
// of the wave (all 64 must execute it), without LDS.  fp32 addition commutes, so both lanes of a pair
// get the same bits and an xor butterfly is the adjacent-pair tree.  The exchanges:
//   X = 1, 2   DPP quad_perm [1,0,3,2] / [2,3,0,1]
//   X = 4      DPP row_half_mirror (lane i of 8 reads 7 - i): the other quad of the 8, whose four
//              lanes hold one value after the X = 1 and 2 levels, which always precede this one
//   X = 8      DPP row_ror:8 (a rotation of the 16-lane row by half of it)
//   X = 16, 32 v_permlane16_swap / v_permlane32_swap of v with itself: the two results are the even
//              and the odd rows' (the lower and the upper half's) value in both of them
template <int X>
__device__ __forceinline__ float ss_add_xor(float v) {
    const int i = __float_as_int(v);
    if constexpr (X < 16) {
        constexpr int kCtrl = X == 1 ? 0xB1 : (X == 2 ? 0x4E : (X == 4 ? 0x141 : 0x128));
        // (every lane of these controls has a source lane: bound_ctrl and the old value never apply,
        // and with them set so the exchange folds into the add as its DPP operand)
        return v + __int_as_float(__builtin_amdgcn_update_dpp(0, i, kCtrl, 0xf, 0xf, true));
    } else if constexpr (X == 16) {
        const auto r = __builtin_amdgcn_permlane16_swap(static_cast<uint32_t>(i), static_cast<uint32_t>(i), false, false);
        return __uint_as_float(r[0]) + __uint_as_float(r[1]);
    } else {
        const auto r = __builtin_amdgcn_permlane32_swap(static_cast<uint32_t>(i), static_cast<uint32_t>(i), false, false);
        return __uint_as_float(r[0]) + __uint_as_float(r[1]);
    }
}
template <int X>
__device__ __forceinline__ void ss_add_xor3(float& r, float& g, float& b) {
    r = ss_add_xor<X>(r); g = ss_add_xor<X>(g); b = ss_add_xor<X>(b);
}
// The tree of a pixel's k x k samples, k = 1 << n (n = 1..3, wave-uniform), in every lane of the pixel:
// the levels along x (lane bits 0..n-1) and then along y (lane bits 3..3+n-1); the wave tile's lanes
// are row-major, px = lane & 7, py = lane >> 3.  One straight line of exchanges per factor.
__device__ __forceinline__ void ss_tree(uint32_t n, float& r, float& g, float& b) {
    ss_add_xor3<1>(r, g, b);
    if (n == 1) {
        ss_add_xor3<8>(r, g, b);
        return;
    }
    ss_add_xor3<2>(r, g, b);
    if (n == 3) ss_add_xor3<4>(r, g, b);
    ss_add_xor3<8>(r, g, b);
    ss_add_xor3<16>(r, g, b);
    if (n == 3) ss_add_xor3<32>(r, g, b);
}

template <bool COUNT, int PHASE, bool DEEP, int SPEC, bool HSTK, bool CULLK, bool SS>
__device__ __forceinline__ void render_tile(const DevScene& S, const FrameArgs& F, uint32_t widx, uint32_t tile,
                                            uint32_t part, uint32_t light, uint4* stk, unsigned long long* sT,
                                            float (*pnum)[64], uint32_t lane) {
    constexpr int kKinds = SPEC & kSpecKindAll;
    constexpr bool kPoint = (SPEC & kSpecPoint) != 0;
    constexpr bool kNoSph = (SPEC & kSpecNoSpheres) != 0, kComb = (SPEC & kSpecCombShadows) != 0;
    constexpr bool kP5 = (SPEC & kSpecFivePlanes) != 0, kOneMesh = (SPEC & kSpecOneMesh) != 0;
    constexpr bool kNoMesh = (SPEC & kSpecNoMesh) != 0;
    constexpr bool kRoom = (SPEC & kSpecRoomPlanes) != 0 && (SPEC & kSpecFivePlanes) != 0;
    constexpr bool kCullBack = (SPEC & kSpecCullBack) != 0 && !COUNT;
    constexpr bool kStored = PHASE == 8 || PHASE == 9;   // the hit record is a stored hit pass's (the planes)
    // the rays' merged domain test (norm_ray3), but for the generic shadow pass without the cull: its two more
    // SGPRs are the kernel's 101st and 102nd, and it would run 7 waves per SIMD for 8
    constexpr bool kDomOne = RTX_FIX_DOMAIN && !(PHASE == 9 && SPEC == 0 && !CULLK);
#if RTX_STAMPS
    // diagnostic build only: per-wave {start, end, hw_id} in the counters buffer
    const unsigned long long t_start = __builtin_amdgcn_s_memrealtime();
    unsigned long long t_prim = t_start, t_shadow = 0;   // primary hit done; shadow mesh walks
#endif
    if constexpr (HSTK) {   // this wave's stacks in HBM
        stk = S.hstk + static_cast<size_t>(widx) * S.hstk_depth;
        if (COUNT) sT = S.hstkT + static_cast<size_t>(widx) * S.hstk_depth;
    }
    const uint32_t slot = widx * 64u + lane;                 // heavy-pixel slot (PHASE > 0)
    const uint32_t per_view = F.tiles_x * F.tiles_y;
    const uint32_t view = tile / per_view;
    const uint32_t rem = tile - view * per_view;
    const uint32_t bx = rem % F.tiles_x;
    const ViewCam& V = F.cam[view];
    uint32_t gy = rem / F.tiles_x;
    unsigned long long t_block0 = 0;
    if (F.cost || ((PHASE == 1 || PHASE == 2) && F.part_max)) t_block0 = __builtin_amdgcn_s_memtime();
    if (F.groups_per_stripe) {
        // view v owns the stripes s with s % step == (first - v) mod step (rtx.h)
        const uint32_t first = (F.stripe_first + F.stripe_step - view % F.stripe_step) % F.stripe_step;
        const uint32_t k = gy / F.groups_per_stripe, sub = gy % F.groups_per_stripe;
        gy = (first + k * F.stripe_step) * F.groups_per_stripe + sub;
    }
    const int px = static_cast<int>(bx * kWaveTile + (lane & 7u));
    const int py = static_cast<int>(gy * kWaveTile + (lane >> 3));
    const bool valid = px < static_cast<int>(F.width) && py < static_cast<int>(F.height);
    Counts cnt;
    if (COUNT || RTX_STAMPS) for (int k = 0; k < kNumCounters; ++k) cnt.c[k] = 0;
    if (COUNT && valid) cnt.c[kPixels] = 1;

    // ---- primary ray
    RTX_PRIMARY_DIR(F, V, kDomOne);
    const unsigned long long vslow = dslow;
    const Ray vr = make_ray(V.origin[0], V.origin[1], V.origin[2], dx, dy, dz, dix, diy, diz, 0.0001f, FLT_MAX);
    const unsigned long long active = ballot(valid);
    // FAST: every active lane's inverse direction finite and non-zero (make_ray's domain)
    const bool fast = (active & vslow) == 0 && S.tri_fast;
    // octant of the wave's primary rays (-1: mixed signs, or no octant copies)
    const int poct = (fast && S.oct_bytes && (PHASE == 0 || PHASE == 4 || PHASE == 7)) ? batch_octant(vr, active) : -1;
    // exact cull of the view's camera anchor (FAST waves; a direction normalised from a magnitude
    // of at least 2^-30 has |d| = 1 +- 3u, which the bound assumes)
    constexpr bool kCull = CULLK && !RTX_STAMPS_WALK;   // (with COUNT: rtx_count_work_culled)
    const bool pcull = kCull && S.cull_stride && fast && (PHASE == 0 || PHASE == 1 || PHASE == 4 || PHASE == 7);
    CullRay pq{};
    if (pcull)
        pq = cull_ray(S.cull + static_cast<size_t>(uni(view)) * (S.cull_stride / 16u), vr, dm >= 0x1p-30f,
                      F.cam[uni(view)].cull_bt);

    // ---- Scene::GetClosestHit (Scene.cpp:29-66)
    float best_t = FLT_MAX, sc_t = FLT_MAX;
    // kind: 0 none, 1 sphere, 2 plane, 3 triangle; best_idx: the record's BYTE offset
    uint32_t best_kind = 0, best_idx = 0;
    // (PHASE 5 reads the hit record PHASE 4 wrote, PHASE 8 the hit pass's: no closest-hit work)
    for (uint32_t i = 0; i < ((PHASE == 5 || PHASE == 6 || kStored) ? 0u : n_sph * 16u); i += 16u) {
        const float4 s = ldcb16(S.spheres, opaque(i));
        if (COUNT && valid) cnt.c[kSphere]++;
        const SphereProj q = sphere_perp(s, vr);
        const unsigned long long near = ballot(!(s.w < q.perp)) & active;
        if (!near) continue;
        const float t = sphere_t(s, q);
        const bool h = ((near >> lane) & 1ull) & !(t < vr.tmin) & !(t > vr.tmax);
        sc_t = h ? t : sc_t;
        const bool b = h & (t < best_t);
        best_t = b ? t : best_t;
        best_kind = b ? 1u : best_kind;
        best_idx = b ? i : best_idx;
    }
    // the room's planes as a / d (room_a), for a wave whose ray origins are finite.  The camera
    // numerators come from the host (ViewCam::room_a); in a FAST wave every d is inside div_rn's
    // divisor domain with its RN(1/d) already in the ray, so when the host found the numerators
    // inside theirs too, t = RN(a / d) costs 3 VALU instead of the 11 of IEEE `/`.
    const bool room_p =
        kRoom && PHASE != 5 && PHASE != 6 && !kStored && !RTX_ABL_PPLANE &&
        (active & ~ballot(finite3(vr.ox, vr.oy, vr.oz))) == 0;
    if (room_p) {
        // the view's record through a readfirstlane'd index: scalar loads (the view index
        // itself stays a VGPR value; making it uniform everywhere measured slower)
        const ViewCam& VU = F.cam[uni(view)];
        const auto room_hit = [&](float t, int k) {
            const bool h = valid & (t >= vr.tmin) & (t < vr.tmax);
            sc_t = h ? t : sc_t;
            const bool b = h & (t < best_t);
            best_t = b ? t : best_t;
            best_kind = b ? 2u : best_kind;
            best_idx = b ? static_cast<uint32_t>(k * 32) : best_idx;
        };
#if RTX_FIX_ROOM
        // the five numerators and room_fast lie side by side in the record: read together ahead of the one
        // branch, they are one scalar fetch and one wait for the wave, not one of each per plane
        const float ra[5] = {VU.room_a[0], VU.room_a[1], VU.room_a[2], VU.room_a[3], VU.room_a[4]};
        if (fast && VU.room_fast) {
            for_room_planes([&](auto kc) {
                constexpr int k = decltype(kc)::value;
                constexpr int A = kRoomAxes[k];
                room_hit(div_rn(ra[k], room_d<A>(vr), room_inv<A>(vr)), k);
            });
        } else {
            for_room_planes([&](auto kc) {
                constexpr int k = decltype(kc)::value;
                constexpr int A = kRoomAxes[k];
                float4 p0, p1;
                ldcb32(S.planes, k * 32u, p0, p1);
                room_hit(room_a<A>(p0, vr) / room_d<A>(vr), k);
            });
        }
#else
        const bool mk = fast && VU.room_fast;
        for_room_planes([&](auto kc) {
            constexpr int k = decltype(kc)::value;
            constexpr int A = kRoomAxes[k];
            float t;
            if (mk) {
                t = div_rn(VU.room_a[k], room_d<A>(vr), room_inv<A>(vr));
            } else {
                float4 p0, p1;
                ldcb32(S.planes, k * 32u, p0, p1);
                t = room_a<A>(p0, vr) / room_d<A>(vr);
            }
            room_hit(t, k);
        });
#endif
    }
    for (uint32_t i = 0; i < ((RTX_ABL_PPLANE || room_p || PHASE == 5 || PHASE == 6 || kStored) ? 0u : n_pl * 32u);
         i += 32u) {
        float4 p0, p1;
        ldcb32(S.planes, opaque(i), p0, p1);
        if (COUNT && valid) cnt.c[kPlane]++;
        const float num = plane_num(p0, p1, vr), den = plane_den(p1, vr);
        const float t = num / den;
        const bool h = valid & (t >= vr.tmin) & (t < vr.tmax);
        sc_t = h ? t : sc_t;
        const bool b = h & (t < best_t);
        best_t = b ? t : best_t;
        best_kind = b ? 2u : best_kind;
        best_idx = b ? i : best_idx;
    }
    if (PHASE == 0 || PHASE == 4 || PHASE == 7) {
        for (uint32_t mi = 0; mi < ((RTX_ABL_PMESH) ? 0u : n_mesh); ++mi) {
            const int4 M = ldcb16i(S.meshes, opaque(mi * 16u));
            uint32_t sc_tri = 0;
            unsigned long long unused = 0;
            if (poct >= 0 && pcull)
                mesh_traverse<false, kSlabOct, COUNT, kCullBack, kCull>(S, M, vr, poct, active, lane, stk, sT, sc_t,
                                                                        sc_tri, unused, cnt, pq);
            else if (poct >= 0)
                mesh_traverse<false, kSlabOct, COUNT, kCullBack>(S, M, vr, poct, active, lane, stk, sT, sc_t, sc_tri,
                                                                 unused, cnt);
            else if (fast && pcull)
                mesh_traverse<false, kSlabFast, COUNT, kCullBack, kCull>(S, M, vr, 0, active, lane, stk, sT, sc_t,
                                                                         sc_tri, unused, cnt, pq);
            else if (fast)
                mesh_traverse<false, kSlabFast, COUNT, kCullBack>(S, M, vr, 0, active, lane, stk, sT, sc_t, sc_tri,
                                                                  unused, cnt);
            else
                mesh_traverse<false, kSlabExact, COUNT, kCullBack>(S, M, vr, 0, active, lane, stk, sT, sc_t, sc_tri,
                                                                   unused, cnt);
            if (sc_t < best_t) { best_t = sc_t; best_kind = 3; best_idx = sc_tri; }
        }
#if RTX_STAMPS
        t_prim = __builtin_amdgcn_s_memrealtime();
#endif
    } else if (PHASE == 1) {
        // one frontier part; sc0 = the scratch t the reference enters the meshes with
        const int4 E = ldc(S.parts, part);
        if (RTX_P1_SHARED_T && valid) {
            // the parts that finished before this one already merged their keys: a lane's final t
            // is at most their minimum T, so the walk needs only hits with t <= T (initial scratch t
            // = the next float above T; equal t still compete on the triangle index).  Read at the
            // coherence point (the keys' atomics come from every XCD); a stale key is larger, still
            // a bound.
            const unsigned long long k0 = __hip_atomic_load(&F.hit_key[slot], __ATOMIC_RELAXED,
                                                             __HIP_MEMORY_SCOPE_AGENT);
            const float tb = __uint_as_float(static_cast<uint32_t>(k0 >> 32) + 1u);
            if (k0 != ~0ull && tb < sc_t) sc_t = tb;
        }
        const float sc0 = sc_t;
        uint32_t sc_tri = 0;
        unsigned long long unused = 0;
        const int oct = (fast && S.oct_bytes) ? batch_octant(vr, active) : -1;
        const bool timed = F.part_cost && F.cost;
        unsigned long long wdt;
        if (oct >= 0 && pcull)
            wdt = part_traverse<false, kSlabOct, kCullBack, kCull>(S, E, vr, oct, active, lane, stk, sc_t, sc_tri,
                                                                   unused, cnt, nullptr, 0u, pq, timed);
        else if (oct >= 0)
            wdt = part_traverse<false, kSlabOct, kCullBack>(S, E, vr, oct, active, lane, stk, sc_t, sc_tri, unused,
                                                            cnt, nullptr, 0u, CullRay{}, timed);
        else if (fast && pcull)
            wdt = part_traverse<false, kSlabFast, kCullBack, kCull>(S, E, vr, 0, active, lane, stk, sc_t, sc_tri,
                                                                    unused, cnt, nullptr, 0u, pq, timed);
        else if (fast)
            wdt = part_traverse<false, kSlabFast, kCullBack>(S, E, vr, 0, active, lane, stk, sc_t, sc_tri, unused,
                                                             cnt, nullptr, 0u, CullRay{}, timed);
        else
            wdt = part_traverse<false, kSlabExact, kCullBack>(S, E, vr, 0, active, lane, stk, sc_t, sc_tri, unused,
                                                              cnt, nullptr, 0u, CullRay{}, timed);
        if (valid && sc_t < sc0)   // accepted t >= tmin > 0: the float bits order like the values
            atomicMin(&F.hit_key[slot], (static_cast<unsigned long long>(__float_as_uint(sc_t)) << 32) | sc_tri);
        if (timed && lane == 0 && wdt) part_cost_add(F.cost + tile, wdt);
        part_stat<PHASE>(F, part, widx, lane, t_block0);
        RTX_SPLIT_STAMP();
        return;
    } else if (PHASE == 2 || PHASE == 3) {
        // the minimum over the parts; strict < against the sphere/plane winner, as after
        // every mesh in Scene::GetClosestHit (Scene.cpp:56-63)
        const unsigned long long key = F.hit_key[slot];
        const float T = __uint_as_float(static_cast<uint32_t>(key >> 32));
        if (key != ~0ull && T < best_t) { best_t = T; best_kind = 3; best_idx = static_cast<uint32_t>(key); }
    }

    // ---- hit record (rebuilt from t: ray.origin + t * ray.direction, Utils.h:62-64)
    bool did = best_kind != 0;
    float hx = 0.f, hy = 0.f, hz = 0.f, nx = 0.f, ny = 0.f, nz = 0.f;
    uint32_t mat = 0;
    const size_t lm_slot = 2 * (static_cast<size_t>(tile) * 64u + lane);   // (PHASE 4/5) the pixel's record
    if (PHASE == 5 || PHASE == 6) {   // PHASE 4's record of this pixel (the previous launch: visible)
        const float4 r0 = F.lm_rec[lm_slot], r1 = F.lm_rec[lm_slot + 1];
        hx = r0.x; hy = r0.y; hz = r0.z; nx = r0.w; ny = r1.x; nz = r1.y;
        mat = __float_as_uint(r1.z);
        did = __float_as_uint(r1.w) != 0u;
    } else if (kStored) {
        // Deferred shading and the shadow pass: closestHit from the stored hit pass (rtx.h, rtx_aov_planes).
        // Lanes outside the frame load nothing and hit nothing; the material index is clamped before any material
        // load, whatever the planes hold (a stale pass, planes the caller edited).
        if (valid) {
            const size_t o = static_cast<size_t>(view) * F.width * F.height + static_cast<size_t>(py) * F.width +
                             static_cast<size_t>(px);
            did = F.aov_primitive[o] != 0u;
            best_t = F.aov_depth[o];
            nx = F.aov_normal[3 * o]; ny = F.aov_normal[3 * o + 1]; nz = F.aov_normal[3 * o + 2];
            const uint32_t m = F.aov_material[o], top = S.n_materials - 1u;
            mat = m < top ? m : top;
        }
        if (did) { hx = vr.ox + vr.dx * best_t; hy = vr.oy + vr.dy * best_t; hz = vr.oz + vr.dz * best_t; }
    } else if (did) {
        hx = vr.ox + vr.dx * best_t; hy = vr.oy + vr.dy * best_t; hz = vr.oz + vr.dz * best_t;
        if ((!RTX_FIX_HIT || !kNoSph) && best_kind == 1) {   // (no sphere arm in a variant without spheres)
            const float4 s = ldcb16(S.spheres, best_idx);
            nx = hx - s.x; ny = hy - s.y; nz = hz - s.z;
            const float m = sqrtf(nx * nx + ny * ny + nz * nz);   // closestHit.normal.Normalize()
            div3_exact(nx, ny, nz, m);   // nx /= m; ny /= m; nz /= m
            mat = ldc(S.sphere_mat, best_idx >> 4);
        } else if (best_kind == 2) {
            float4 p0, p1;
            ldcb32(S.planes, best_idx, p0, p1);
            nx = p1.x; ny = p1.y; nz = p1.z;
            mat = __float_as_uint(p0.w);
        } else {
            Tri T;
            ldcb64(S.tris, best_idx, T.a, T.b, T.c, T.d);   // best_idx: byte offset
            nx = T.a.w; ny = T.b.w; nz = T.c.w;
            mat = __float_as_uint(T.d.x);
        }
    }
    if (COUNT && did) cnt.c[kHit]++;
    if (PHASE == 4) {   // light-major: the record for PHASE 5, and this wave's share of the tile's cost
        F.lm_rec[lm_slot] = make_float4(hx, hy, hz, nx);
        F.lm_rec[lm_slot + 1] = make_float4(ny, nz, __uint_as_float(mat), __uint_as_float(did ? 1u : 0u));
        if (F.cost && lane == 0) part_cost_add(F.cost + tile, __builtin_amdgcn_s_memtime() - t_block0);
        return;
    }

    if (PHASE == 7) {   // hit pass: the record in the caller's terms (rtx.h, rtx_aov_planes), no colour
        if (valid) {
            const size_t o = static_cast<size_t>(view) * F.width * F.height + static_cast<size_t>(py) * F.width +
                             static_cast<size_t>(px);
            const uint32_t m = uni(F.aov_mask);
            if (m & RTX_AOV_DEPTH) F.aov_depth[o] = best_t;   // (a miss: the empty HitRecord's FLT_MAX)
            if (m & RTX_AOV_NORMAL) {
                F.aov_normal[3 * o] = nx; F.aov_normal[3 * o + 1] = ny; F.aov_normal[3 * o + 2] = nz;
            }
            if (m & RTX_AOV_MATERIAL) F.aov_material[o] = mat;
            // best_idx is the record's byte offset: 16 B per sphere, 32 per plane, 64 per triangle
            if (m & RTX_AOV_PRIMITIVE)
                F.aov_primitive[o] = did ? (best_kind << 30) | (best_idx >> (best_kind + 3u)) : 0u;
        }
        return;
    }

    float shadowFactor = 1.f;
    float fr = 0.f, fg = 0.f, fb = 0.f;
    const unsigned long long hitmask = ballot(did);
    unsigned long long lm_occ = 0;   // PHASE 5: the lanes whose shadow ray toward `light` is occluded
    uint32_t sh_bits = 0;            // PHASE 9: bit l = this lane's shadow ray toward light l is occluded
    // The reference's light loop (Renderer.cpp:128-176).  Light-major frames run it in two launches:
    // PHASE 5 casts its one light's shadow ray and only records the occluded lanes; PHASE 6 (lm_shade)
    // runs it over every light with each light's occlusion the one PHASE 5 published
    // (FrameArgs::lm_mask), no shadow ray cast.
    constexpr bool lm_shade = PHASE == 6;
    if (hitmask) {
        // PHASE 9: the lights to trace are a wave-uniform mask (FrameArgs::lm_lights, rtx_kernels.h), and the loop
        // runs from its lowest to its highest set bit: the first light, which fills the plane-numerator
        // cache below, is the first traced one
        uint32_t sh_trace = 0u;
        if constexpr (PHASE == 9) sh_trace = uni(F.lm_lights);
        const uint32_t l_first = (PHASE == 2 || PHASE == 5) ? light
                                 : (PHASE == 9 && sh_trace) ? static_cast<uint32_t>(__builtin_ctz(sh_trace)) : 0u;
        const uint32_t l_end = (PHASE == 2 || PHASE == 5) ? light + 1
                               : PHASE == 9 ? (sh_trace ? 32u - static_cast<uint32_t>(__builtin_clz(sh_trace)) : 0u)
                                            : (RTX_ABL_LIGHTS ? 0u : S.n_lights);
        // originOffset = hit.origin + hit.normal * 0.0001f (Renderer.cpp:126)
        const float oox = hx + nx * 0.0001f, ooy = hy + ny * 0.0001f, ooz = hz + nz * 0.0001f;
        const float vx = -dx, vy = -dy, vz = -dz;
        // Room skip: a wave whose shadow origins all lie strictly inside the room, every light being
        // strictly inside it too (the host's fact, rtx_upload.hip room_skip), runs no shadow-ray plane
        // test, because the reference's own binary32 test (HitTest_Plane on Ray{o, d, 1e-4, tmax},
        // l = RN(L - o) per component, tmax = |l| as computed, d = RN(l / tmax)) provably fails.
        // Plane k, axis A, normal component s = +-1; exact alpha = s * (o_A - p0_A), exact margin
        // m = s * (L_A - p0_A) >= mmin > 0; the lane condition is s * a < 0 for a = RN(p0_A - o_A) (the
        // sign of a binary32 difference is exact: alpha > 0) and |a| <= M <= 2^20 * mmin; u = 2^-24.
        //   * o is finite (|a| <= M), so the reference's num and den are s * a and s * d_A (room_a).
        //     A hit needs t = RN(a / d_A) >= tmin > 0: d_A non-zero with s * d_A < 0.  d_A has the sign of
        //     l_A (tmax > 0) and l_A that of the exact L_A - o_A, so s * (L_A - o_A) = m - alpha < 0 and
        //     |L_A - o_A| = alpha - m: the ray approaches the plane, and the light lies before it.
        //   * tmax = 0 makes d infinite and t = 0 < tmin; tmax = inf makes d_A = 0 and t infinite or
        //     NaN.  Otherwise tmax is a positive float, whatever the rounding, underflow or contraction
        //     in its sum of squares: d_A was divided by the same float that t is compared with.
        //   * t < tmax fails when |a| >= |d_A| * tmax, RN being monotone and tmax a float.  |d_A| =
        //     RN(|l_A| / tmax) <= (|l_A| / tmax)(1 + u) + 2^-150 (the second term: a denormal or zero
        //     d_A), |l_A| <= (alpha - m)(1 + u) and |a| >= alpha (1 - u) (a denormal difference is
        //     exact), so it suffices that
        //         alpha (1 - u) - (alpha - m)(1 + u)^2 >= 2^-150 tmax,
        //     whose left side is at least m - alpha (3u + u^2) >= m (1 - 2^20 (1 + 2u)(3u + u^2)) > 0.8 m,
        //     since alpha <= |a| / (1 - u) <= 2^20 (1 + 2u) m: the roundings take 3/16 of m at 2^20.
        //   * the right side: every axis B has a plane, so |L_B - o_B| <= (its margin) + (its alpha) <=
        //     (2^20 + 2) mmax, and tmax <= sqrt(3)(1 + 3u)(2^20 + 2) mmax < 2^21 mmax (squares that
        //     underflow only leave tmax < 2^-61, and m >= 2^-149 as a non-zero difference of floats).
        //     The host's fact requires mmax <= 2^100 mmin, hence 2^-150 tmax < 2^-29 m.
        // The lane condition is an interval per axis, found on the host by evaluating it (room_skip):
        // the record behind the planes is {lo, M}, {hi, 0}, empty (lo = +inf, hi = -inf) when the fact
        // does not hold, and a NaN or infinite coordinate fails the compares, so room_clear implies
        // room_s's finiteness.  6 VALU per pixel for 15 plane tests in the headline.
        bool room_clear = false;
        if constexpr (kRoom && !COUNT && PHASE != 2 && !RTX_ABL_SPLANE) {
            float4 q0, q1;
            ldcb32(S.planes, 5 * 32u, q0, q1);
            const bool inside = (q0.x < oox) & (oox < q1.x) & (q0.y < ooy) & (ooy < q1.y) & (q0.z < ooz) & (ooz < q1.z);
            room_clear = (hitmask & ~ballot(inside)) == 0;
        }
        // shadow rays start at originOffset for every light: one finiteness test for all of them
        const bool room_s = kRoom && PHASE != 2 && !RTX_ABL_SPLANE && !room_clear &&
                            (hitmask & ~ballot(finite3(oox, ooy, ooz))) == 0;
        for (uint32_t li = l_first; li < l_end; ++li) {
            if (PHASE == 9 && !((sh_trace >> li) & 1u)) continue;   // (scalar: a light outside the trace mask)
            float4 L0, L1;
            ldcb32(S.lights, opaque(li * 32u), L0, L1);
            const int ltype = kPoint ? RTX_LIGHT_POINT : __float_as_int(L0.w);
            RTX_LIGHT_DIR(kDomOne);
            bool occ = false;
            if (lm_shade && f_shadows) {   // PHASE 6: published by the previous launch
                const unsigned long long mk = F.lm_mask[static_cast<size_t>(tile) * F.lm_lights + li];
                occ = did && ((mk >> lane) & 1ull);
            } else if (f_shadows) {
                // Scene::DoesHit (Scene.cpp:68-96) on Ray{originOffset, l, 1e-4, |l|}; `live` =
                // lanes still without an occluder (first hit wins, order irrelevant for a bool)
                const unsigned long long sslow = lslow;
                const Ray sr = make_ray(oox, ooy, ooz, lx, ly, lz, lix, liy, liz, 0.0001f, mag);
                unsigned long long live = hitmask;
                const bool sfast = (hitmask & sslow) == 0 && S.tri_fast;
                const int soct =
                    (sfast && S.oct_bytes && (PHASE == 0 || PHASE == 5 || kStored) && n_mesh) ? batch_octant(sr, hitmask)
                                                                                              : -1;
                // exact cull of the light's anchor: lanes with mag <= cull_T[li] (and a direction
                // normalised from at least 2^-30)
                const bool scull =
                    kCull && S.cull_stride && sfast && (PHASE == 0 || PHASE == 2 || PHASE == 5 || kStored) && n_mesh;
                CullRay sq{};
                if (scull)
                    sq = cull_ray(S.cull + static_cast<size_t>(kMaxViews + li) * (S.cull_stride / 16u), sr,
                                  mag >= 0x1p-30f && mag <= ldc(S.cull_T, li), ldc(S.cull_T, li));
                if (COUNT && did) cnt.c[kShadow]++;
                // (single-condition loops with a separate exit test: a `&& live` loop
                // condition is carried as a VGPR boolean by the compiler)
                for (uint32_t i = 0; i < (PHASE == 2 ? 0u : n_sph * 16u); i += 16u) {
                    const float4 s = ldcb16(S.spheres, opaque(i));
                    if (COUNT && ((live >> lane) & 1ull)) cnt.c[kSphere]++;
                    const SphereProj q = sphere_perp(s, sr);
                    const unsigned long long near = ballot(!(s.w < q.perp)) & live;
                    if (!near) continue;
                    const float t = sphere_t(s, q);
                    live &= ~(near & ballot(!(t < sr.tmin)) & ballot(!(t > sr.tmax)));
                }
                // HitTest_Plane's numerator (p0 - o) . n depends only on the shadow ray's origin,
                // the same originOffset for every light: the first light computes it and keeps it
                // in LDS, the others read it back (same value, bit for bit).  One loop version
                // per case, so no per-plane select.
                const uint32_t np = (RTX_ABL_SPLANE || PHASE == 2 || room_s || room_clear) ? 0u : n_pl * 32u;
                const bool cache_ok = !COUNT && np <= static_cast<uint32_t>(kPlaneCache) * 32u;
                if (room_clear) {   // no room plane can occlude any light (room skip, above)
                } else if (room_s) {   // a / d (room_a): cheaper than the cached numerator
                    for_room_planes([&](auto kc) {
                        constexpr int k = decltype(kc)::value;
                        constexpr int A = kRoomAxes[k];
                        float4 p0, p1;
                        ldcb32(S.planes, k * 32u, p0, p1);
                        const float num = room_a<A>(p0, sr), den = room_d<A>(sr);
                        const unsigned long long cand = plane_cand(num, den, sr.tmax) & live;
                        if (!cand) return;
                        const float t = num / den;
                        live &= ~(ballot(t >= sr.tmin) & ballot(t < sr.tmax) & cand);
                    });
                } else if (cache_ok && li != l_first) {
                    for (uint32_t i = 0; i < np; i += 32u) {
                        float4 p0, p1;
                        ldcb32(S.planes, opaque(i), p0, p1);
                        const float num = pnum[i >> 5][lane];
                        const float den = plane_den(p1, sr);
                        const unsigned long long cand = plane_cand(num, den, sr.tmax) & live;
                        if (!cand) continue;
                        const float t = num / den;
                        live &= ~(ballot(t >= sr.tmin) & ballot(t < sr.tmax) & cand);
                    }
                } else {
                    for (uint32_t i = 0; i < np; i += 32u) {
                        float4 p0, p1;
                        ldcb32(S.planes, opaque(i), p0, p1);
                        if (COUNT && ((live >> lane) & 1ull)) cnt.c[kPlane]++;
                        const float num = plane_num(p0, p1, sr), den = plane_den(p1, sr);
                        if (cache_ok) pnum[i >> 5][lane] = num;
                        const unsigned long long cand = plane_cand(num, den, sr.tmax) & live;
                        if (!cand) continue;   // also taken once no lane is live
                        const float t = num / den;
                        live &= ~(ballot(t >= sr.tmin) & ballot(t < sr.tmax) & cand);
                    }
                }
#if RTX_STAMPS
                const unsigned long long ts0 = __builtin_amdgcn_s_memrealtime();
#endif
                for (uint32_t mi = 0; mi < ((RTX_ABL_SMESH || !(PHASE == 0 || PHASE == 5 || kStored)) ? 0u : n_mesh); ++mi) {
                    if (!live) break;
                    float st = 0.f;
                    uint32_t stri = 0;
                    const int4 M = ldcb16i(S.meshes, opaque(mi * 16u));
                    if (soct >= 0 && scull)
                        mesh_traverse<true, kSlabOct, COUNT, kCullBack, kCull>(S, M, sr, soct, live, lane, stk, sT, st,
                                                                               stri, live, cnt, sq);
                    else if (soct >= 0)
                        mesh_traverse<true, kSlabOct, COUNT, kCullBack>(S, M, sr, soct, live, lane, stk, sT, st, stri,
                                                                        live, cnt);
                    else if (sfast && scull)
                        mesh_traverse<true, kSlabFast, COUNT, kCullBack, kCull>(S, M, sr, 0, live, lane, stk, sT, st,
                                                                                stri, live, cnt, sq);
                    else if (sfast)
                        mesh_traverse<true, kSlabFast, COUNT, kCullBack>(S, M, sr, 0, live, lane, stk, sT, st, stri,
                                                                         live, cnt);
                    else
                        mesh_traverse<true, kSlabExact, COUNT, kCullBack>(S, M, sr, 0, live, lane, stk, sT, st, stri,
                                                                          live, cnt);
                }
#if RTX_STAMPS
                t_shadow += __builtin_amdgcn_s_memrealtime() - ts0;
#endif
                if (PHASE == 2) {
                    const int4 E = ldc(S.parts, part);
                    float st = 0.f;
                    uint32_t stri = 0;
                    const int poct2 = (sfast && S.oct_bytes) ? batch_octant(sr, hitmask) : -1;
                    const bool timed = F.part_cost && F.cost;
                    unsigned long long wdt;
                    if (poct2 >= 0 && scull)
                        wdt = part_traverse<true, kSlabOct, kCullBack, kCull>(S, E, sr, poct2, live, lane, stk, st, stri,
                                                                              live, cnt, &F.occ_bits[slot], 1u << li, sq,
                                                                              timed);
                    else if (poct2 >= 0)
                        wdt = part_traverse<true, kSlabOct, kCullBack>(S, E, sr, poct2, live, lane, stk, st, stri, live,
                                                                       cnt, &F.occ_bits[slot], 1u << li, CullRay{}, timed);
                    else if (sfast && scull)
                        wdt = part_traverse<true, kSlabFast, kCullBack, kCull>(S, E, sr, 0, live, lane, stk, st, stri,
                                                                               live, cnt, &F.occ_bits[slot], 1u << li, sq,
                                                                               timed);
                    else if (sfast)
                        wdt = part_traverse<true, kSlabFast, kCullBack>(S, E, sr, 0, live, lane, stk, st, stri, live, cnt,
                                                                        &F.occ_bits[slot], 1u << li, CullRay{}, timed);
                    else
                        wdt = part_traverse<true, kSlabExact, kCullBack>(S, E, sr, 0, live, lane, stk, st, stri, live,
                                                                         cnt, &F.occ_bits[slot], 1u << li, CullRay{}, timed);
                    if (did && !((live >> lane) & 1ull)) atomicOr(&F.occ_bits[slot], 1u << li);
                    if (timed && lane == 0 && wdt) part_cost_add(F.cost + tile, wdt);
                    continue;
                }
                occ = did & !((live >> lane) & 1ull);
                if (PHASE == 3) occ = occ || (did && ((F.occ_bits[slot] >> li) & 1u));
            }
            if (PHASE == 5) {
                lm_occ = ballot(occ);
                continue;
            }
            if (PHASE == 9) {   // the shadow pass keeps DoesHit's answer for every light and shades nothing
                sh_bits |= (occ ? 1u : 0u) << li;
                continue;
            }
            if (!did) continue;
            if (occ) {
                if (COUNT) cnt.c[kOccluded]++;
                shadowFactor *= 0.95f;
                continue;
            }
            if (COUNT) cnt.c[kShadeBase]++;
            RTX_LIGHT_TERM(f_mode, kKinds, COUNT)
        }
        if (did && PHASE != 5) { fr *= shadowFactor; fg *= shadowFactor; fb *= shadowFactor; }
    }
    if (PHASE == 9) {   // the shadow plane's word (rtx_render_shadows_async): a miss and a lightless scene store 0
        // An update (rtx_update_shadows_async) carries the untraced lights' bits over: new = (old & keep) |
        // traced, keep in FrameArgs::heavy_n.  The full pass has keep = 0 and never reads the plane.
        const uint32_t keep = uni(F.heavy_n);
        if (valid) {
            const size_t o = static_cast<size_t>(view) * F.width * F.height + static_cast<size_t>(py) * F.width +
                             static_cast<size_t>(px);
            F.occ_bits[o] = sh_bits | (keep ? F.occ_bits[o] & keep : 0u);
        }
        return;
    }
    if (PHASE == 5) {   // the light's occluded lanes for PHASE 6
        if (lane == 0) F.lm_mask[static_cast<size_t>(tile) * F.lm_lights + light] = lm_occ;
        if (F.cost && lane == 0) part_cost_add(F.cost + tile, __builtin_amdgcn_s_memtime() - t_block0);
        return;
    }
    if (PHASE == 2) {
        part_stat<PHASE>(F, part, widx, lane, t_block0);
        RTX_SPLIT_STAMP();
        return;
    }
    if (PHASE == 3) {   // ready for the next frame's split launches
        F.hit_key[slot] = ~0ull;
        F.occ_bits[slot] = 0u;
    }
    RTX_MAX_TO_ONE()
    if constexpr (SS) {
        // Supersampled frame: this lane's sample is (px & (k - 1), py & (k - 1)) of pixel (px / k, py / k),
        // k = 1 << ss_log2 dividing the tile's 8, so the wave holds every sample of its pixels and a
        // pixel's samples are valid together.  The box filter: per channel the adjacent-pair tree over
        // sx, then over sy, times the exact 1 / (k * k); the pixel's first lane stores it.
        const uint32_t n = uni(F.ss_log2);
        ss_tree(n, fr, fg, fb);
        const float w = __uint_as_float((127u - 2u * n) << 23);   // 2^(-2 log2 k)
        fr *= w; fg *= w; fb *= w;
        const uint32_t m = (1u << n) - 1u;
        if (valid && ((lane | (lane >> 3)) & m) == 0) {
            const size_t o = (static_cast<size_t>(view) * F.out_height + (static_cast<uint32_t>(py) >> n)) * F.out_width +
                             (static_cast<uint32_t>(px) >> n);
            F.out_px[o] = RTX_PACK_PX(F);
            if (F.out_rgb) {
                F.out_rgb[3 * o] = fr; F.out_rgb[3 * o + 1] = fg; F.out_rgb[3 * o + 2] = fb;
            }
        }
    } else if (valid) {
        const size_t o = static_cast<size_t>(view) * F.width * F.height + static_cast<size_t>(py) * F.width +
                         static_cast<size_t>(px);
        F.out_px[o] = RTX_PACK_PX(F);
        if (F.out_rgb) {
            F.out_rgb[3 * o] = fr; F.out_rgb[3 * o + 1] = fg; F.out_rgb[3 * o + 2] = fb;
        }
    }
    if (PHASE == 0 && F.cost && lane == 0) {   // split tiles keep their one-piece cost
        const unsigned long long dt = (__builtin_amdgcn_s_memtime() - t_block0) >> 4;
        atomicMax(&F.cost[tile], static_cast<uint32_t>(dt < 0xffffffffull ? dt : 0xffffffffull));
    }
    // light-major: the tile's cost is the sum of its waves' (PHASE 4 + every light wave)
    if ((PHASE == 5 || PHASE == 6) && F.cost && lane == 0)
        part_cost_add(F.cost + tile, __builtin_amdgcn_s_memtime() - t_block0);
#if RTX_STAMPS
    if (PHASE == 0 && lane == 0 && F.stamps) {
        const unsigned long long t_end = __builtin_amdgcn_s_memrealtime();
        const size_t w = tile;
        unsigned hw;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        unsigned xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        unsigned long long* st = F.stamps + kStampWords * w;
        st[0] = t_start;
        st[1] = t_end;
        st[2] = (static_cast<unsigned long long>(xcc) << 32) | hw;
        st[3] = cnt.c[kWaveNodeTests];
        st[4] = cnt.c[kWaveTriTests];
        st[5] = (static_cast<unsigned long long>(cnt.c[kSlab]) << 32) | cnt.c[kTri];
        st[6] = t_prim - t_start;
        st[7] = t_shadow;
    }
#endif
    if (COUNT) {
        for (int k = 0; k < kNumCounters; ++k)
            if (cnt.c[k]) atomicAdd(&F.counters[k], static_cast<unsigned long long>(cnt.c[k]));
    }
}


// The one SS variant built for 7 waves per SIMD where its plain twin has 8: PHASE 0 of the Lambert +
// Cook-Torrance one-mesh kernel with the cull (W4_Optional) fills the 64 VGPRs of 8 waves exactly, and
// the SS epilogue's one more live VGPR put 3 VGPRs into scratch around the light loop.
template <int PHASE, int SPEC, bool CULLK, bool SS>
constexpr bool kSsSevenWaves = SS && CULLK && PHASE == 0 && (SPEC & kSpecKindCT) != 0 && (SPEC & kSpecOneMesh) != 0;

template <bool COUNT, int PHASE, bool DEEP = false, int SPEC = 0, bool HSTK = false, bool CULLK = false,
          bool SS = false>
__global__ void __launch_bounds__(kBlockThreads, (DEEP && !HSTK) ? 2
                                                  : ((SPEC & (kSpecOneMesh | kSpecNoMesh))
                                                         ? (kSsSevenWaves<PHASE, SPEC, CULLK, SS> ? RTX_SPEC_WAVES_PARTIAL
                                                                                                  : RTX_SPEC_WAVES)
                                                         : (SPEC ? RTX_SPEC_WAVES_PARTIAL : RTX_MIN_WAVES_PER_EU)))
    rtx_render_kernel(const DevScene S, const FrameArgs F) {
    constexpr int kDepth = HSTK ? 1 : (DEEP ? kStackDepthDeep : kStackDepth);
    __shared__ uint4 stkE[kBlockThreads / 64][kDepth];
    __shared__ unsigned long long stkT[(COUNT && !HSTK) ? kBlockThreads / 64 : 1][(COUNT && !HSTK) ? kDepth : 1];
    // per-lane shadow-ray plane numerators, shared by every light (see the light loop)
    __shared__ float pnumS[kBlockThreads / 64][kPlaneCache][64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint4* stk = stkE[wave];
    unsigned long long* sT = stkT[COUNT ? wave : 0];

    // Work unit = one 8x8 wave tile of one view; the waves of a workgroup (one by default,
    // RTX_BLOCK_THREADS) are independent (no barrier) and take consecutive entries of the
    // dispatch order.  The order is a permutation (F.order, null = identity) that
    // rtx_reorder_kernel derives from the previous frame's measured per-tile cost: heavy
    // tiles start first and do not form a tail.  One-wave workgroups free their slot the
    // moment the wave ends (4-wave ones held it until the slowest sibling ended: Bunny
    // -3 %, Synthetic100k -9 %).  Which wave renders a tile never changes a pixel's value.
    const uint32_t b = blockIdx.x;
    uint32_t widx = b * kWavesPerBlock + wave;   // wave index in the launch
    uint32_t tile, part = 0, light = 0;
    // PHASE 4/5: the light-major frame (FrameArgs::lm_*): PHASE 4 = PHASE 0 up to the hit record,
    // PHASE 5 = item (tile, light), the tiles in dispatch order and a tile's lights consecutive
    if (PHASE == 0 || PHASE == 4 || PHASE == 6 || PHASE == 7 || PHASE == 8 || PHASE == 9) {
        if (widx >= F.n_tiles) return;
        tile = F.order ? ldc(F.order, widx) : widx;
        if (F.heavy_flag && ldc(F.heavy_flag, tile)) return;   // rendered by the split launches
    } else if (PHASE == 5) {
        // persistent waves, one per resident wave slot: wave w takes items w, w + NW, w + 2 NW, ... of the
        // cost-ordered list, so every wave gets a share of the heavy items and no per-item workgroup is
        // dispatched (130k one-wave workgroups at 4K / 8 ranks cost more to launch than to run)
        const uint32_t L = F.lm_lights, items = F.n_tiles * L, nw = gridDim.x * kWavesPerBlock;
        for (uint32_t it = uni(widx); it < items; it += nw) {   // (wave-uniform: the light indexes scalar loads)
            const uint32_t k = it / L;
            tile = F.order ? ldc(F.order, k) : k;
            if (F.heavy_flag && ldc(F.heavy_flag, tile)) continue;
            render_tile<COUNT, PHASE, DEEP, SPEC, HSTK, CULLK, SS>(S, F, it, tile, 0u, it - k * L, stk, sT, pnumS[wave],
                                                               lane);
        }
        return;
    } else {
        // grid (heavy tiles / waves per block, parts, lights), tile fastest: every heavy tile's part 0 is
        // dispatched first, the big top-of-tree parts before the small ones.  (Pinning a
        // part to one XCD for L2 locality was measured slower: the heavy parts then load a
        // few XCDs only.)
        if (widx >= F.heavy_n) return;
        part = blockIdx.y;
        light = blockIdx.z;
        tile = ldc(F.heavy_list, widx);
    }
    render_tile<COUNT, PHASE, DEEP, SPEC, HSTK, CULLK, SS>(S, F, widx, tile, part, light, stk, sT, pnumS[wave], lane);
}

#undef f_mode
#undef f_shadows
#undef n_sph
#undef n_pl
#undef n_mesh

// ====================================================================== the ray kernels' shared bodies
// Scene::GetClosestHit, Scene::DoesHit, the hit record and the reference's light loop for a ray that is
// not render_tile's: rtx_query_kernel, rtx_shade_kernel and rtx_adaptive_kernel (below) all call these,
// so each body is stated once for the three.  They share every test and walk with the render kernel
// (sphere_perp / sphere_t, plane_num / plane_den, mesh_traverse and below, shade, the RTX_LIGHT_* macros)
// but not these loops: with the loops as helpers called from render_tile too, 94 of the render kernel's
// instantiations compiled to other code (tools/codeobj_diff.py).  So the helpers stand after render_tile,
// which never calls them and is the parent's instruction for instruction
// (profiles/ray_kernels_shared/codeobj_diff.txt).
// The renderer's own shortcuts stay off here: no exact cull (its records are anchored at a camera or a
// light, and a caller's ray has no anchor), no room a / d planes or room skip, no camera numerators, no
// LDS numerator cache, no atomicMin key, no split phases.  sphere_perp / sphere_t, plane_num / plane_den,
// the hit record's rebuild and div3_exact restate the reference for any operand.
namespace {

// A caller's ray: eight floats (rtx_ray), read with vector loads.  A tail lane keeps a harmless ray; it
// is in no mask.
struct QRay {
    float v[8];
};
__device__ __forceinline__ Ray load_ray(const float* __restrict__ rays, uint32_t i, bool valid,
                                        unsigned long long& slow) {
    QRay q = {{0.f, 0.f, 0.f, 1.f, 1.f, 1.f, 1.f, 0.f}};
    if (valid) q = *reinterpret_cast<const QRay*>(rays + static_cast<size_t>(i) * 8u);
    return make_ray(q.v[0], q.v[1], q.v[2], q.v[3], q.v[4], q.v[5], q.v[6], q.v[7], slow);
}

// The walk a wave takes.  A ray here is any eight floats (a shadow ray starts wherever a caller's ray
// put the hit point), and the result is the reference's for them, so every shortcut that is proved for
// the renderer's own rays is taken per wave, when all ACTIVE lanes are inside its domain, and the exact
// form otherwise:
//   * rcp3_exact's domain (each |d_k| in [2^-60, 2^60]): make_ray's `slow`.  A slow lane has a zero,
//     infinite or NaN inverse component, and v_min / v_max then drop a NaN that std::min / std::max
//     keep: the wave takes kSlabExact.
//   * a NaN origin makes the same NaN slab values with a finite inverse: non-finite origins count as
//     slow.  (An infinite one gives infinite slab values of either form; it is excluded with them.)
//   * tri_t<FAST> skips the |a| > 2^60 check for |d| < 2 and |e1||e2| <= 2^56 (DevScene::tri_fast), and
//     its reduced cross products equal Vector3::Cross's only while their terms are finite: taken when
//     every active lane is not slow and has |d_k| <= 1 (so |d| <= sqrt 3) and |o_k| <= 2^40, and the scene
//     is tri_fast; otherwise XC, Vector3::Cross as written plus the check.
//   * the octant node copies: a wave that is fast in all of the above, S.oct_bytes, batch_octant >= 0.
struct WaveWalk {
    bool slab_fast, fast;
    int oct;
};
__device__ __forceinline__ WaveWalk wave_walk(const DevScene& S, const Ray& r, unsigned long long slow,
                                              unsigned long long active) {
    slow |= ballot(!finite3(r.ox, r.oy, r.oz));
    WaveWalk w;
    w.slab_fast = (active & slow) == 0;
    const bool tri_dom = fmaxf(fmaxf(fabsf(r.dx), fabsf(r.dy)), fabsf(r.dz)) <= 1.f &&
                         fmaxf(fmaxf(fabsf(r.ox), fabsf(r.oy)), fabsf(r.oz)) <= 0x1p40f;
    // (v_max drops a NaN component, and a lane with one is slow already)
    w.fast = w.slab_fast && S.tri_fast && (active & ~ballot(tri_dom)) == 0;
    w.oct = (w.fast && S.oct_bytes) ? batch_octant(r, active) : -1;
    return w;
}

// One mesh by the wave's walk.  ANY: `mask` is `live`, which loses the occluded lanes.
template <bool ANY>
__device__ __forceinline__ void walk_mesh(const DevScene& S, const int4 M, const Ray& r, const WaveWalk& w,
                                          unsigned long long mask, uint32_t lane, uint4* stk, float& t, uint32_t& tri,
                                          unsigned long long& live, Counts& cnt) {
    if (w.oct >= 0)
        mesh_traverse<ANY, kSlabOct, false>(S, M, r, w.oct, mask, lane, stk, nullptr, t, tri, live, cnt);
    else if (w.fast)
        mesh_traverse<ANY, kSlabFast, false>(S, M, r, 0, mask, lane, stk, nullptr, t, tri, live, cnt);
    else if (w.slab_fast)
        mesh_traverse<ANY, kSlabFast, false, false, false, true>(S, M, r, 0, mask, lane, stk, nullptr, t, tri, live,
                                                                 cnt);
    else
        mesh_traverse<ANY, kSlabExact, false, false, false, true>(S, M, r, 0, mask, lane, stk, nullptr, t, tri, live,
                                                                  cnt);
}

// Scene::DoesHit (Scene.cpp:68-96) for the lanes of `active`; returns `live`, the lanes still without
// an occluder.  plane_cand skips the division for lanes that cannot pass t >= tmin given tmin > 0, and
// its "beyond" test is stated for a finite tmax: taken when every active lane has tmin > 0 and
// |tmax| < inf (NaN fails); otherwise t = num / den is computed and tested as HitTest_Plane does (with
// tmin <= 0 a zero or negative t is a hit).  (A shadow ray has tmin = 1e-4, so its domain is a finite
// tmax = |l| in every hit lane.)
__device__ __forceinline__ unsigned long long any_hit(const DevScene& S, const Ray& r, const WaveWalk& w,
                                                      unsigned long long active, uint32_t lane, uint4* stk,
                                                      Counts& cnt) {
    unsigned long long live = active;
    for (uint32_t k = 0; k < S.n_spheres * 16u; k += 16u) {
        const float4 s = ldcb16(S.spheres, opaque(k));
        const SphereProj p = sphere_perp(s, r);
        const unsigned long long near = ballot(!(s.w < p.perp)) & live;
        if (!near) continue;
        const float t = sphere_t(s, p);
        live &= ~(near & ballot(!(t < r.tmin)) & ballot(!(t > r.tmax)));
    }
    const bool pl_dom = (active & ~ballot(r.tmin > 0.f && fabsf(r.tmax) < INFINITY)) == 0;
    if (pl_dom) {
        for (uint32_t k = 0; k < S.n_planes * 32u; k += 32u) {
            float4 p0, p1;
            ldcb32(S.planes, opaque(k), p0, p1);
            const float num = plane_num(p0, p1, r), den = plane_den(p1, r);
            const unsigned long long cand = plane_cand(num, den, r.tmax) & live;
            if (!cand) continue;   // also taken once no lane is live
            const float t = num / den;
            live &= ~(ballot(t >= r.tmin) & ballot(t < r.tmax) & cand);
        }
    } else {
        for (uint32_t k = 0; k < S.n_planes * 32u; k += 32u) {
            float4 p0, p1;
            ldcb32(S.planes, opaque(k), p0, p1);
            const float t = plane_num(p0, p1, r) / plane_den(p1, r);
            live &= ~(ballot(t >= r.tmin) & ballot(t < r.tmax));
        }
    }
    for (uint32_t mi = 0; mi < S.n_meshes; ++mi) {
        if (!live) break;
        float st = 0.f;
        uint32_t stri = 0;
        const int4 M = ldcb16i(S.meshes, opaque(mi * 16u));
        walk_mesh<true>(S, M, r, w, live, lane, stk, st, stri, live, cnt);
    }
    return live;
}

// Scene::GetClosestHit (Scene.cpp:29-66), as PHASE 7 of render_tile outside the room (the planes always
// divide).  kind: 0 none, 1 sphere, 2 plane, 3 triangle; idx: the record's BYTE offset (16 B per sphere,
// 32 per plane, 64 per triangle); a miss keeps the empty HitRecord's t = FLT_MAX.
struct Closest {
    float t;
    uint32_t kind, idx;
};
__device__ __forceinline__ Closest closest_hit(const DevScene& S, const Ray& r, const WaveWalk& w,
                                               unsigned long long active, bool valid, uint32_t lane, uint4* stk,
                                               Counts& cnt) {
    float best_t = FLT_MAX, sc_t = FLT_MAX;
    uint32_t best_kind = 0, best_idx = 0;
    for (uint32_t k = 0; k < S.n_spheres * 16u; k += 16u) {
        const float4 s = ldcb16(S.spheres, opaque(k));
        const SphereProj p = sphere_perp(s, r);
        const unsigned long long near = ballot(!(s.w < p.perp)) & active;
        if (!near) continue;
        const float t = sphere_t(s, p);
        const bool h = ((near >> lane) & 1ull) & !(t < r.tmin) & !(t > r.tmax);
        sc_t = h ? t : sc_t;
        const bool b = h & (t < best_t);
        best_t = b ? t : best_t;
        best_kind = b ? 1u : best_kind;
        best_idx = b ? k : best_idx;
    }
    for (uint32_t k = 0; k < S.n_planes * 32u; k += 32u) {
        float4 p0, p1;
        ldcb32(S.planes, opaque(k), p0, p1);
        const float t = plane_num(p0, p1, r) / plane_den(p1, r);
        const bool h = valid & (t >= r.tmin) & (t < r.tmax);
        sc_t = h ? t : sc_t;
        const bool b = h & (t < best_t);
        best_t = b ? t : best_t;
        best_kind = b ? 2u : best_kind;
        best_idx = b ? k : best_idx;
    }
    for (uint32_t mi = 0; mi < S.n_meshes; ++mi) {
        const int4 M = ldcb16i(S.meshes, opaque(mi * 16u));
        uint32_t sc_tri = 0;
        unsigned long long unused = 0;
        walk_mesh<false>(S, M, r, w, active, lane, stk, sc_t, sc_tri, unused, cnt);
        if (sc_t < best_t) { best_t = sc_t; best_kind = 3; best_idx = sc_tri; }
    }
    return {best_t, best_kind, best_idx};
}

// The hit record, rebuilt from t (ray.origin + t * ray.direction, Utils.h:62-64).  POINT: hit.origin for
// every hit, as render_tile rebuilds it (the light loop needs it); without, only a sphere's normal does.
struct HitRec {
    float hx, hy, hz, nx, ny, nz;
    uint32_t mat;
};
template <bool POINT>
__device__ __forceinline__ HitRec hit_record(const DevScene& S, const Ray& r, const Closest& c) {
    HitRec h = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0u};
    if (c.kind != 0) {
        if (POINT || c.kind == 1) {
            h.hx = r.ox + r.dx * c.t; h.hy = r.oy + r.dy * c.t; h.hz = r.oz + r.dz * c.t;
        }
        if (c.kind == 1) {
            const float4 s = ldcb16(S.spheres, c.idx);
            h.nx = h.hx - s.x; h.ny = h.hy - s.y; h.nz = h.hz - s.z;
            const float m = sqrtf(h.nx * h.nx + h.ny * h.ny + h.nz * h.nz);   // closestHit.normal.Normalize()
            div3_exact(h.nx, h.ny, h.nz, m);   // nx /= m; ny /= m; nz /= m
            h.mat = ldc(S.sphere_mat, c.idx >> 4);
        } else if (c.kind == 2) {
            float4 p0, p1;
            ldcb32(S.planes, c.idx, p0, p1);
            h.nx = p1.x; h.ny = p1.y; h.nz = p1.z;
            h.mat = __float_as_uint(p0.w);
        } else {
            Tri T;
            ldcb64(S.tris, c.idx, T.a, T.b, T.c, T.d);
            h.nx = T.a.w; h.ny = T.b.w; h.nz = T.c.w;
            h.mat = __float_as_uint(T.d.x);
        }
    }
    return h;
}

// The reference's light loop (Renderer.cpp:128-176) and ColorRGB::MaxToOne for the hit `h` of ray `r`:
// render_tile's generic one (SPEC 0, shade<0>, no counters) in the macros it expands, with viewDirection
// = -direction whatever its length.  The shadow ray Ray{originOffset, l, 1e-4, |l|} runs any_hit with
// `hitmask` as the active mask, by the walk its own slow bits, origin and direction choose.
__device__ __forceinline__ void light_loop(const DevScene& S, const Ray& r, const HitRec& h, bool did, int mode,
                                           int shadows, uint32_t lane, uint4* stk, Counts& cnt, float& fr, float& fg,
                                           float& fb) {
    const float hx = h.hx, hy = h.hy, hz = h.hz, nx = h.nx, ny = h.ny, nz = h.nz;
    const uint32_t mat = h.mat;
    float shadowFactor = 1.f;
    fr = 0.f; fg = 0.f; fb = 0.f;
    const unsigned long long hitmask = ballot(did);
    if (hitmask) {
        // originOffset = hit.origin + hit.normal * 0.0001f (Renderer.cpp:126)
        const float oox = hx + nx * 0.0001f, ooy = hy + ny * 0.0001f, ooz = hz + nz * 0.0001f;
        const float vx = -r.dx, vy = -r.dy, vz = -r.dz;
        for (uint32_t li = 0; li < S.n_lights; ++li) {
            float4 L0, L1;
            ldcb32(S.lights, opaque(li * 32u), L0, L1);
            const int ltype = __float_as_int(L0.w);
            RTX_LIGHT_DIR(bool(RTX_FIX_DOMAIN));
            bool occ = false;
            if (shadows) {
                const unsigned long long sslow = lslow;
                const Ray sr = make_ray(oox, ooy, ooz, lx, ly, lz, lix, liy, liz, 0.0001f, mag);
                const WaveWalk sw = wave_walk(S, sr, sslow, hitmask);
                const unsigned long long live = any_hit(S, sr, sw, hitmask, lane, stk, cnt);
                occ = did & !((live >> lane) & 1ull);
            }
            if (!did) continue;
            if (occ) {
                shadowFactor *= 0.95f;
                continue;
            }
            RTX_LIGHT_TERM(mode, 0, false)
        }
        if (did) { fr *= shadowFactor; fg *= shadowFactor; fb *= shadowFactor; }
    }
    RTX_MAX_TO_ONE()
}

}  // namespace

// ====================================================================== ray queries
// Scene::GetClosestHit (ANY = false) and Scene::DoesHit (ANY = true) on caller-supplied rays
// (rtx_trace_rays*, rtx_occluded*, rtx.h): rays 64w .. 64w + 63 are wave w, ray i lane i & 63, tail
// lanes inactive; one wave is one workgroup.  Closest hit is the hit pass (PHASE 7 of render_tile) with
// the ray read from memory and a linear output index (closest_hit, hit_record); occlusion is any_hit on
// the lane's own ray over the wave's active mask.  DEEP / HSTK: the DFS stacks, as in the render kernel.
template <bool ANY, bool DEEP, bool HSTK>
__global__ void __launch_bounds__(kBlockThreads, (DEEP && !HSTK) ? 2 : RTX_MIN_WAVES_PER_EU)
    rtx_query_kernel(const DevScene S, const QueryArgs Q) {
    constexpr int kDepth = HSTK ? 1 : (DEEP ? kStackDepthDeep : kStackDepth);
    __shared__ uint4 stkE[kBlockThreads / 64][kDepth];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t widx = blockIdx.x * kWavesPerBlock + wave;
    if (widx * 64u >= Q.n) return;
    uint4* stk = stkE[wave];
    if constexpr (HSTK) stk = S.hstk + static_cast<size_t>(widx) * S.hstk_depth;
    const uint32_t i = widx * 64u + lane;
    const bool valid = i < Q.n;
    unsigned long long slow;
    const Ray r = load_ray(Q.rays, i, valid, slow);
    const unsigned long long active = ballot(valid);
    const WaveWalk w = wave_walk(S, r, slow, active);
    Counts cnt;   // (never counted: the walks' COUNT is off)

    if constexpr (ANY) {
        const unsigned long long live = any_hit(S, r, w, active, lane, stk, cnt);
        if (valid) Q.occ[i] = static_cast<uint8_t>(((live >> lane) & 1ull) ? 0u : 1u);
    } else {
        const Closest c = closest_hit(S, r, w, active, valid, lane, stk, cnt);
        const HitRec h = hit_record<false>(S, r, c);
        if (valid) {
            const size_t o = i;
            const uint32_t m = uni(Q.mask);
            if (m & RTX_AOV_DEPTH) Q.depth[o] = c.t;   // (a miss: the empty HitRecord's FLT_MAX)
            if (m & RTX_AOV_NORMAL) {
                Q.normal[3 * o] = h.nx; Q.normal[3 * o + 1] = h.ny; Q.normal[3 * o + 2] = h.nz;
            }
            if (m & RTX_AOV_MATERIAL) Q.material[o] = h.mat;
            // c.idx is the record's byte offset: 16 B per sphere, 32 per plane, 64 per triangle
            if (m & RTX_AOV_PRIMITIVE) Q.primitive[o] = c.kind != 0 ? (c.kind << 30) | (c.idx >> (c.kind + 3u)) : 0u;
        }
    }
}

// ====================================================================== shaded rays
// Renderer::RenderPixel from GetClosestHit on (Renderer.cpp:116-181) for caller-supplied rays
// (rtx_shade_rays*, rtx.h): the ray is the caller's eight floats as rtx_query_kernel reads them, in its
// layout (ray i = lane i & 63 of wave i / 64, tail lanes inactive and storing nothing), and viewDirection
// is the ray's direction as given, so Material::Shade receives -direction whatever its length.
// The body is the ray kernels' shared one: closest_hit, hit_record with hit.origin, light_loop.
// Occupancy target: the generic kernel's (65 VGPRs, 7 waves per SIMD).  Asked for 8 waves the default
// kernel fits 64 VGPRs without scratch and measured 2-3 % slower on W4_Bunny and W3 at 1080p
// (profiles/shade/ab_waves8.txt), and the HBM-stack one spilled.
template <bool DEEP, bool HSTK>
__global__ void __launch_bounds__(kBlockThreads, (DEEP && !HSTK) ? 2 : RTX_MIN_WAVES_PER_EU)
    rtx_shade_kernel(const DevScene S, const ShadeArgs Q) {
    constexpr int kDepth = HSTK ? 1 : (DEEP ? kStackDepthDeep : kStackDepth);
    __shared__ uint4 stkE[kBlockThreads / 64][kDepth];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t widx = blockIdx.x * kWavesPerBlock + wave;
    if (widx * 64u >= Q.n) return;
    uint4* stk = stkE[wave];
    if constexpr (HSTK) stk = S.hstk + static_cast<size_t>(widx) * S.hstk_depth;
    const uint32_t i = widx * 64u + lane;
    const bool valid = i < Q.n;
    unsigned long long slow;
    const Ray r = load_ray(Q.rays, i, valid, slow);
    const unsigned long long active = ballot(valid);
    const WaveWalk w = wave_walk(S, r, slow, active);
    Counts cnt;   // (never counted: the walks' COUNT is off)

    const Closest c = closest_hit(S, r, w, active, valid, lane, stk, cnt);
    const HitRec h = hit_record<true>(S, r, c);
    float fr, fg, fb;
    light_loop(S, r, h, c.kind != 0, Q.mode, Q.shadows, lane, stk, cnt, fr, fg, fb);
    if (valid) {
        const size_t o = i;
        if (Q.out_px) Q.out_px[o] = (q8(fr) << Q.rshift) | (q8(fg) << Q.gshift) | (q8(fb) << Q.bshift) | Q.amask;
        if (Q.out_rgb) {
            Q.out_rgb[3 * o] = fr; Q.out_rgb[3 * o + 1] = fg; Q.out_rgb[3 * o + 2] = fb;
        }
    }
}

// ====================================================================== adaptive supersampling
// The refinement of rtx_render_adaptive* (rtx.h): for each pixel rtx_classify_kernel listed
// (AdaptiveArgs::list, y << 16 | x; their number in AdaptiveArgs::count, read from the device), the k x k
// samples of rtx_set_supersample's contract rendered and resolved into the frame buffer; no other pixel is
// written.
// Lanes: a wave holds 64 / k^2 listed pixels; lane bits 0 .. n-1 are sx, the next n bits sy (n = log2 k),
// the rest the pixel's slot, so a pixel's lanes are valid together.  Tail lanes carry the shade kernel's
// harmless ray and are in no mask.
// The lane's ray is render_tile's primary ray of sample (k x + sx, k y + sy) of the k W x k H frame, in
// the macro it expands; from there on the body is rtx_shade_kernel's, the ray kernels' shared one (the
// generic walks chosen per wave, SPEC 0, no exact cull, no room planes).
// The resolve is the butterfly ss_add_xor3<1>, <2>, <4>, <8>, <16>, <32> cut after 2 n levels: with this
// layout the first n levels are the contract's adjacent-pair tree over sx and the next n the tree over
// sy.  <4> (row_half_mirror) equals lane ^ 4 only once a quad's four lanes hold one value: it is level 3
// of k = 4 and k = 8, after <1> and <2>, and k = 2 ends before it.  The loop is wave-uniform, so all 64
// lanes execute every level.
// Grid: persistent waves, wave w takes items w, w + NW, ... (an item = one wave's pixels); the host sizes
// NW from the device's wave slots, never from W * H * k^2.  HSTK: one stack per wave of the grid.
template <bool DEEP, bool HSTK>
__global__ void __launch_bounds__(kBlockThreads, (DEEP && !HSTK) ? 2 : RTX_MIN_WAVES_PER_EU)
    rtx_adaptive_kernel(const DevScene S, const AdaptiveArgs A) {
    constexpr int kDepth = HSTK ? 1 : (DEEP ? kStackDepthDeep : kStackDepth);
    __shared__ uint4 stkE[kBlockThreads / 64][kDepth];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t widx = blockIdx.x * kWavesPerBlock + wave;
    uint4* stk = stkE[wave];
    if constexpr (HSTK) stk = S.hstk + static_cast<size_t>(widx) * S.hstk_depth;
    const uint32_t n = A.ss_log2, km = (1u << n) - 1u;
    const uint32_t ppw_log2 = 6u - 2u * n;   // a wave's pixels: 16, 4, 1
    const uint32_t count = ldc(A.count, 0);
    const uint32_t items = (count + (1u << ppw_log2) - 1u) >> ppw_log2;
    const uint32_t nw = gridDim.x * kWavesPerBlock;
    for (uint32_t it = uni(widx); it < items; it += nw) {
        // (from an opaque copy of the lane index: recomputed per item, not kept across the loop)
        uint32_t l1 = lane;
        asm volatile("" : "+v"(l1));
        const uint32_t sx = l1 & km, sy = (l1 >> n) & km, slot = l1 >> (2u * n);
        const uint32_t i = (it << ppw_log2) + slot;
        const bool valid = i < count;
        uint32_t xy = 0;
        if (valid) xy = A.list[i];
        const int px = static_cast<int>(((xy & 0xffffu) << n) | sx);
        const int py = static_cast<int>(((xy >> 16) << n) | sy);

        // ---- primary ray (Renderer.cpp:104-114), as render_tile makes it for the sample frame
        RTX_PRIMARY_DIR(A, A, bool(RTX_FIX_DOMAIN));
        unsigned long long slow;
        // (a tail lane keeps the shade kernel's harmless ray; it is in no mask)
        const Ray r = make_ray(valid ? A.origin[0] : 0.f, valid ? A.origin[1] : 0.f, valid ? A.origin[2] : 0.f,
                               valid ? dx : 1.f, valid ? dy : 1.f, valid ? dz : 1.f, valid ? 0.0001f : 1.f,
                               valid ? FLT_MAX : 0.f, slow);
        const unsigned long long active = ballot(valid);
        const WaveWalk w = wave_walk(S, r, slow, active);
        Counts cnt;   // (never counted: the walks' COUNT is off)

        const Closest c = closest_hit(S, r, w, active, valid, lane, stk, cnt);
        const HitRec h = hit_record<true>(S, r, c);
        float fr, fg, fb;
        light_loop(S, r, h, c.kind != 0, A.mode, A.shadows, lane, stk, cnt, fr, fg, fb);

        // ---- the box filter: the sx tree, then the sy tree, times the exact 1 / (k * k)
        ss_add_xor3<1>(fr, fg, fb);
        ss_add_xor3<2>(fr, fg, fb);
        if (n >= 2) {
            ss_add_xor3<4>(fr, fg, fb);
            ss_add_xor3<8>(fr, fg, fb);
        }
        if (n == 3) {
            ss_add_xor3<16>(fr, fg, fb);
            ss_add_xor3<32>(fr, fg, fb);
        }
        const float wgt = __uint_as_float((127u - 2u * n) << 23);   // 2^(-2 log2 k)
        fr *= wgt; fg *= wgt; fb *= wgt;
        // the pixel's sample 0 stores; its list entry is read again from an opaque copy of the lane index,
        // so that neither it nor the sample coordinates stay in registers through the body above
        uint32_t l2 = lane;
        asm volatile("" : "+v"(l2));
        const uint32_t i2 = (it << ppw_log2) + (l2 >> (2u * n));
        if (i2 < count && (l2 & ((1u << (2u * n)) - 1u)) == 0) {
            const uint32_t xy2 = A.list[i2];
            const size_t o = static_cast<size_t>(xy2 >> 16) * A.out_width + (xy2 & 0xffffu);
            A.out_px[o] = (q8(fr) << A.rshift) | (q8(fg) << A.gshift) | (q8(fb) << A.bshift) | A.amask;
            if (A.out_rgb) {
                A.out_rgb[3 * o] = fr; A.out_rgb[3 * o + 1] = fg; A.out_rgb[3 * o + 2] = fb;
            }
        }
    }
}

// ====================================================================== relighting
// Renderer::RenderPixel from originOffset on (Renderer.cpp:126-181) for a stored hit pass whose shadow
// rays are stored too (rtx_relight*, rtx.h): PHASE 8 with DoesHit replaced by the pixel's bit of the shadow
// plane, so no ray is cast, nothing is walked, and the kernel needs neither LDS nor a stack.  One lane per
// pixel, a wave = 64 consecutive pixels of a row (RelightArgs), so the five plane loads and the stores are
// full-width; the view, the row and the lights are wave-uniform (cameras and lights come by scalar loads).
// The arithmetic is render_tile's by construction: RTX_PRIMARY_DIR, RTX_LIGHT_DIR, RTX_LIGHT_TERM (with the
// generic shade<0>: a specialised variant compiles the same operations for the kinds its scene has),
// RTX_MAX_TO_ONE and RTX_PACK_PX are the text render_tile expands, over div_rn, div3_exact, shade, smax and
// q8, the functions it calls; the hit point's rebuild is worded as PHASE 8 words it.  The material index is
// clamped as in PHASE 8; a lane outside the row loads and stores nothing.
__global__ void __launch_bounds__(kRelightThreads) rtx_relight_kernel(const DevScene S, const RelightArgs A) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t widx = uni(blockIdx.x * (kRelightThreads / 64u) + (threadIdx.x >> 6));
    const uint32_t per_view = A.segs * A.rows;
    if (widx >= per_view * A.n_views) return;
    const uint32_t view = widx / per_view;
    const uint32_t rem = widx - view * per_view;
    const uint32_t j = rem / A.segs, seg = rem - j * A.segs;
    unsigned long long row = j;
    if (A.stripe_rows) {
        // view v owns the stripes s with s % step == (first - v) mod step (rtx.h)
        const uint32_t first = (A.stripe_first + A.stripe_step - view % A.stripe_step) % A.stripe_step;
        const uint32_t k = j / A.stripe_rows, sub = j % A.stripe_rows;
        row = (first + static_cast<unsigned long long>(k) * A.stripe_step) * A.stripe_rows + sub;
    }
    if (row >= A.height) return;
    const ViewCam& V = A.cam[view];
    const int px = static_cast<int>(seg * 64u + lane), py = static_cast<int>(row);
    const bool valid = px < static_cast<int>(A.width);
    RTX_PRIMARY_DIR(A, V, bool(RTX_FIX_DOMAIN));
    (void)dm;

    // ---- closestHit from the planes, as PHASE 8 reads it
    const size_t o = static_cast<size_t>(view) * A.width * A.height + static_cast<size_t>(py) * A.width +
                     static_cast<size_t>(px);
    bool did = false;
    float t = FLT_MAX, nx = 0.f, ny = 0.f, nz = 0.f;
    float hx = 0.f, hy = 0.f, hz = 0.f;
    uint32_t mat = 0, bits = 0;
    if (valid) {
        did = A.primitive[o] != 0u;
        t = A.depth[o];
        nx = A.normal[3 * o]; ny = A.normal[3 * o + 1]; nz = A.normal[3 * o + 2];
        const uint32_t m = A.material[o], top = S.n_materials - 1u;
        mat = m < top ? m : top;
        if (A.shadows) bits = A.shadow[o];
    }
    if (did) { hx = V.origin[0] + dx * t; hy = V.origin[1] + dy * t; hz = V.origin[2] + dz * t; }

    // ---- the reference's light loop (Renderer.cpp:128-176), DoesHit answered by the shadow plane
    float shadowFactor = 1.f;
    float fr = 0.f, fg = 0.f, fb = 0.f;
    Counts cnt;   // (never counted)
    if (ballot(did)) {
        const float oox = hx + nx * 0.0001f, ooy = hy + ny * 0.0001f, ooz = hz + nz * 0.0001f;
        const float vx = -dx, vy = -dy, vz = -dz;
        for (uint32_t li = 0; li < S.n_lights; ++li) {
            float4 L0, L1;
            ldcb32(S.lights, opaque(li * 32u), L0, L1);
            const int ltype = __float_as_int(L0.w);
            RTX_LIGHT_DIR(bool(RTX_FIX_DOMAIN));
            (void)mag;   // (the shadow ray's tmax: no ray here)
            if (!did) continue;
            // (with shadows on the host has checked the plane's light count against the scene's, at most 32)
            if (A.shadows && li < 32u && ((bits >> li) & 1u)) {
                shadowFactor *= 0.95f;
                continue;
            }
            RTX_LIGHT_TERM(A.mode, 0, false)
        }
        if (did) { fr *= shadowFactor; fg *= shadowFactor; fb *= shadowFactor; }
    }
    RTX_MAX_TO_ONE()
    if (valid) {
        A.out_px[o] = RTX_PACK_PX(A);
        if (A.out_rgb) {
            A.out_rgb[3 * o] = fr; A.out_rgb[3 * o + 1] = fg; A.out_rgb[3 * o + 2] = fb;
        }
    }
}

// The resolved relight (rtx_relight_resolve*, rtx.h): the stored hit pass is the k*W x k*H sample frame of a
// W x H frame (K = 1 << N, N = 1..3), each sample is shaded exactly as rtx_relight_kernel shades a pixel (the
// same macros over the sample frame's RelightArgs, up to and including RTX_MAX_TO_ONE), and the k x k samples
// of an output pixel are resolved with rtx_set_supersample's box filter: per channel the adjacent-pair tree
// over sx, then over sy, times the exact 1 / (k * k).
// A wave is 64 consecutive samples of one sample row, as in rtx_relight_kernel, so every plane load stays a
// full-width row piece; 64 is a multiple of K, so the wave holds whole pixels and a pixel's K lanes are inside
// the row together.  It walks the K sample rows of ONE output row (A.rows, A.stripe_* and the row rule count
// OUTPUT rows here): each iteration is the relight body for one sample row, then the x tree over lane bits
// 0..N-1 (ss_add_xor<1>, <2>, <4>, the DPP exchanges of the supersampled frame; every lane of the wave
// executes them: a lane outside the row loads and stores nothing but never returns early), then the y tree in
// registers in pair order, (r0 + r1), (r2 + r3), then pairs of those: row sy is added to the pending sum of each
// level whose bit of sy is set, and parked at the first level whose bit is clear (sy is wave-uniform, so these
// are scalar branches and the pending sums are 3 N registers).  The lane with lane % K == 0 stores the pixel.
// No LDS, no scratch, no stack.
template <int N>
__global__ void __launch_bounds__(kRelightThreads, N < 3 ? RTX_RESOLVE_WAVES : RTX_MIN_WAVES_PER_EU)
rtx_relight_resolve_kernel(const DevScene S, const RelightArgs A) {
    constexpr uint32_t K = 1u << N;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t widx = uni(blockIdx.x * (kRelightThreads / 64u) + (threadIdx.x >> 6));
    const uint32_t per_view = A.segs * A.rows;
    if (widx >= per_view * A.n_views) return;
    const uint32_t view = widx / per_view;
    const uint32_t rem = widx - view * per_view;
    const uint32_t j = rem / A.segs, seg = rem - j * A.segs;
    const uint32_t out_w = A.width >> N, out_h = A.height >> N;
    unsigned long long orow = j;
    if (A.stripe_rows) {
        // view v owns the stripes s with s % step == (first - v) mod step (rtx.h), in output rows
        const uint32_t first = (A.stripe_first + A.stripe_step - view % A.stripe_step) % A.stripe_step;
        const uint32_t k = j / A.stripe_rows, sub = j % A.stripe_rows;
        orow = (first + static_cast<unsigned long long>(k) * A.stripe_step) * A.stripe_rows + sub;
    }
    if (orow >= out_h) return;   // (wave-uniform)
    const ViewCam& V = A.cam[view];
    const int px = static_cast<int>(seg * 64u + lane);
    const bool valid = px < static_cast<int>(A.width);
    float p0r = 0.f, p0g = 0.f, p0b = 0.f, p1r = 0.f, p1g = 0.f, p1b = 0.f, p2r = 0.f, p2g = 0.f, p2b = 0.f;
    float fr = 0.f, fg = 0.f, fb = 0.f;
#pragma unroll 1
    for (uint32_t sy = 0; sy < K; ++sy) {
        const int py = static_cast<int>(static_cast<uint32_t>(orow) * K + sy);
        RTX_PRIMARY_DIR(A, V, bool(RTX_FIX_DOMAIN));
        (void)dm;

        // ---- closestHit from the planes, as PHASE 8 reads it
        const size_t o = static_cast<size_t>(view) * A.width * A.height + static_cast<size_t>(py) * A.width +
                         static_cast<size_t>(px);
        bool did = false;
        float t = FLT_MAX, nx = 0.f, ny = 0.f, nz = 0.f;
        float hx = 0.f, hy = 0.f, hz = 0.f;
        uint32_t mat = 0, bits = 0;
        if (valid) {
            did = A.primitive[o] != 0u;
            t = A.depth[o];
            nx = A.normal[3 * o]; ny = A.normal[3 * o + 1]; nz = A.normal[3 * o + 2];
            const uint32_t m = A.material[o], top = S.n_materials - 1u;
            mat = m < top ? m : top;
            if (A.shadows) bits = A.shadow[o];
        }
        if (did) { hx = V.origin[0] + dx * t; hy = V.origin[1] + dy * t; hz = V.origin[2] + dz * t; }

        // ---- the reference's light loop (Renderer.cpp:128-176), DoesHit answered by the shadow plane
        float shadowFactor = 1.f;
        fr = 0.f; fg = 0.f; fb = 0.f;
        Counts cnt;   // (never counted)
        if (ballot(did)) {
            const float oox = hx + nx * 0.0001f, ooy = hy + ny * 0.0001f, ooz = hz + nz * 0.0001f;
            const float vx = -dx, vy = -dy, vz = -dz;
            for (uint32_t li = 0; li < S.n_lights; ++li) {
                float4 L0, L1;
                ldcb32(S.lights, opaque(li * 32u), L0, L1);
                const int ltype = __float_as_int(L0.w);
                RTX_LIGHT_DIR(bool(RTX_FIX_DOMAIN));
                (void)mag;   // (the shadow ray's tmax: no ray here)
                if (!did) continue;
                if (A.shadows && li < 32u && ((bits >> li) & 1u)) {
                    shadowFactor *= 0.95f;
                    continue;
                }
                RTX_LIGHT_TERM(A.mode, 0, false)
            }
            if (did) { fr *= shadowFactor; fg *= shadowFactor; fb *= shadowFactor; }
        }
        RTX_MAX_TO_ONE()
        // ---- the x tree: this sample row's K samples of each pixel, in every lane of the pixel
        ss_add_xor3<1>(fr, fg, fb);
        if constexpr (N >= 2) ss_add_xor3<2>(fr, fg, fb);
        if constexpr (N >= 3) ss_add_xor3<4>(fr, fg, fb);
        // ---- the y tree: rows in adjacent pairs, then pairs of pairs
        if (!(sy & 1u)) { p0r = fr; p0g = fg; p0b = fb; continue; }
        fr = p0r + fr; fg = p0g + fg; fb = p0b + fb;
        if constexpr (N >= 2) {
            if (!(sy & 2u)) { p1r = fr; p1g = fg; p1b = fb; continue; }
            fr = p1r + fr; fg = p1g + fg; fb = p1b + fb;
        }
        if constexpr (N >= 3) {
            if (!(sy & 4u)) { p2r = fr; p2g = fg; p2b = fb; continue; }
            fr = p2r + fr; fg = p2g + fg; fb = p2b + fb;
        }
    }
    (void)p1r; (void)p1g; (void)p1b; (void)p2r; (void)p2g; (void)p2b;   // (levels a smaller K does not have)
    const float w = __uint_as_float((127u - 2u * N) << 23);   // 2^(-2 log2 k)
    fr *= w; fg *= w; fb *= w;
    if (valid && (lane & (K - 1u)) == 0u) {
        const size_t o = (static_cast<size_t>(view) * out_h + static_cast<size_t>(orow)) * out_w +
                         (static_cast<uint32_t>(px) >> N);
        A.out_px[o] = RTX_PACK_PX(A);
        if (A.out_rgb) {
            A.out_rgb[3 * o] = fr; A.out_rgb[3 * o + 1] = fg; A.out_rgb[3 * o + 2] = fb;
        }
    }
}

#undef RTX_PRIMARY_DIR
#undef RTX_LIGHT_DIR
#undef RTX_LIGHT_TERM
#undef RTX_MAX_TO_ONE
#undef RTX_PACK_PX

// ====================================================================== launches
namespace {

// The split launches of a frame (PHASE 1-3) in the frame's specialised variant v (-1: generic).
template <int P, bool CU, bool SS>
void launch_phase_v(int v, dim3 g, hipStream_t s, const DevScene& d, const FrameArgs& F) {
    switch (v) {
    case 0: hipLaunchKernelGGL((rtx_render_kernel<false, P, false, kSpecVariants[0], false, CU, SS>), g, dim3(kBlockThreads), 0, s, d, F); break;
    case 1: hipLaunchKernelGGL((rtx_render_kernel<false, P, false, kSpecVariants[1], false, CU, SS>), g, dim3(kBlockThreads), 0, s, d, F); break;
    case 2: hipLaunchKernelGGL((rtx_render_kernel<false, P, false, kSpecVariants[2], false, false, SS>), g, dim3(kBlockThreads), 0, s, d, F); break;   // (no mesh: nothing to cull)
    case 3: hipLaunchKernelGGL((rtx_render_kernel<false, P, false, kSpecVariants[3], false, CU, SS>), g, dim3(kBlockThreads), 0, s, d, F); break;
    case 4: hipLaunchKernelGGL((rtx_render_kernel<false, P, false, kSpecVariants[4], false, CU, SS>), g, dim3(kBlockThreads), 0, s, d, F); break;
    default: hipLaunchKernelGGL((rtx_render_kernel<false, P, false, 0, false, CU, SS>), g, dim3(kBlockThreads), 0, s, d, F); break;
    }
}
// ... of a supersampled frame (FrameArgs::ss_log2) in the SS instantiation when P has the output
// epilogue (PHASE 0, 3 and 6; the other phases are the same code for every factor)
template <int P, bool CU>
void launch_phase_s(int v, dim3 g, hipStream_t s, const DevScene& d, const FrameArgs& F) {
    constexpr bool kOut = P == 0 || P == 3 || P == 6;
    if (kOut && F.ss_log2) launch_phase_v<P, CU, kOut>(v, g, s, d, F);
    else launch_phase_v<P, CU, false>(v, g, s, d, F);
}
// PHASE P of a frame in the frame's specialised variant v (-1: generic), with the cull variant
// when the scene has cull records
template <int P>
void launch_phase(int v, dim3 g, hipStream_t s, const DevScene& d, const FrameArgs& F) {
    if (d.cull_stride) launch_phase_s<P, true>(v, g, s, d, F);
    else launch_phase_s<P, false>(v, g, s, d, F);
}

// The one-launch frames without a specialised variant (the counting and the deep-stack kernels), in
// the SS instantiation for a supersampled frame.
template <bool COUNT, bool DEEP, bool HSTK, bool CU>
void launch_one(dim3 g, hipStream_t s, const DevScene& d, const FrameArgs& F) {
    if (F.ss_log2)
        hipLaunchKernelGGL((rtx_render_kernel<COUNT, 0, DEEP, 0, HSTK, CU, true>), g, dim3(kBlockThreads), 0, s, d, F);
    else
        hipLaunchKernelGGL((rtx_render_kernel<COUNT, 0, DEEP, 0, HSTK, CU>), g, dim3(kBlockThreads), 0, s, d, F);
}

[[noreturn]] void no_instantiation(const char* what) {
    std::fprintf(stderr, "librtx_hip: no rtx_render_kernel instantiation for %s\n", what);
    std::abort();
}

}  // namespace

namespace rtxh {

void launch_render_phase(int phase, int variant, dim3 grid, hipStream_t s, const DevScene& d, const FrameArgs& F) {
    switch (phase) {
    case 0: launch_phase<0>(variant, grid, s, d, F); break;
    case 1: launch_phase<1>(variant, grid, s, d, F); break;
    case 2: launch_phase<2>(variant, grid, s, d, F); break;
    case 3: launch_phase<3>(variant, grid, s, d, F); break;
    case 4: launch_phase<4>(variant, grid, s, d, F); break;
    case 5: launch_phase<5>(variant, grid, s, d, F); break;
    case 6: launch_phase<6>(variant, grid, s, d, F); break;
    default: no_instantiation("this phase");
    }
}

void launch_render_one(bool count, bool deep, bool hstk, bool cull, dim3 grid, hipStream_t s, const DevScene& d,
                       const FrameArgs& F) {
    switch ((count ? 8 : 0) | (deep ? 4 : 0) | (hstk ? 2 : 0) | (cull ? 1 : 0)) {
    case 8 | 1: launch_one<true, false, false, true>(grid, s, d, F); break;
    case 8 | 4 | 2: launch_one<true, true, true, false>(grid, s, d, F); break;
    case 8 | 4: launch_one<true, true, false, false>(grid, s, d, F); break;
    case 8: launch_one<true, false, false, false>(grid, s, d, F); break;
    case 4 | 2: launch_one<false, true, true, false>(grid, s, d, F); break;
    case 4: launch_one<false, true, false, false>(grid, s, d, F); break;
    default: no_instantiation("this one-launch frame");
    }
}

void launch_hit_pass(bool deep, bool hstk, bool cull, dim3 grid, hipStream_t s, const DevScene& d, const FrameArgs& F) {
    switch ((deep ? 4 : 0) | (hstk ? 2 : 0) | (cull ? 1 : 0)) {
    case 4 | 2: hipLaunchKernelGGL((rtx_render_kernel<false, 7, true, 0, true>), grid, dim3(kBlockThreads), 0, s, d, F); break;
    case 4: hipLaunchKernelGGL((rtx_render_kernel<false, 7, true>), grid, dim3(kBlockThreads), 0, s, d, F); break;
    case 1: hipLaunchKernelGGL((rtx_render_kernel<false, 7, false, 0, false, true>), grid, dim3(kBlockThreads), 0, s, d, F); break;
    case 0: hipLaunchKernelGGL((rtx_render_kernel<false, 7>), grid, dim3(kBlockThreads), 0, s, d, F); break;
    default: no_instantiation("this hit pass");
    }
}

void launch_deferred(int variant, bool deep, bool hstk, dim3 grid, hipStream_t s, const DevScene& d, const FrameArgs& F) {
    if (hstk) hipLaunchKernelGGL((rtx_render_kernel<false, 8, true, 0, true>), grid, dim3(kBlockThreads), 0, s, d, F);
    else if (deep) hipLaunchKernelGGL((rtx_render_kernel<false, 8, true>), grid, dim3(kBlockThreads), 0, s, d, F);
    else launch_phase<8>(variant, grid, s, d, F);
}

void launch_shadows(int variant, bool deep, bool hstk, dim3 grid, hipStream_t s, const DevScene& d, const FrameArgs& F) {
    if (hstk) hipLaunchKernelGGL((rtx_render_kernel<false, 9, true, 0, true>), grid, dim3(kBlockThreads), 0, s, d, F);
    else if (deep) hipLaunchKernelGGL((rtx_render_kernel<false, 9, true>), grid, dim3(kBlockThreads), 0, s, d, F);
    else launch_phase<9>(variant, grid, s, d, F);
}

void launch_relight(dim3 grid, hipStream_t s, const DevScene& d, const RelightArgs& A) {
    hipLaunchKernelGGL(rtx_relight_kernel, grid, dim3(kRelightThreads), 0, s, d, A);
}

void launch_relight_resolve(uint32_t ss_log2, dim3 grid, hipStream_t s, const DevScene& d, const RelightArgs& A) {
    switch (ss_log2) {
    case 1: hipLaunchKernelGGL(rtx_relight_resolve_kernel<1>, grid, dim3(kRelightThreads), 0, s, d, A); break;
    case 2: hipLaunchKernelGGL(rtx_relight_resolve_kernel<2>, grid, dim3(kRelightThreads), 0, s, d, A); break;
    case 3: hipLaunchKernelGGL(rtx_relight_resolve_kernel<3>, grid, dim3(kRelightThreads), 0, s, d, A); break;
    default: no_instantiation("this resolve factor");
    }
}

template <bool ANY>
static void launch_query_t(bool deep, bool hstk, dim3 grid, hipStream_t s, const DevScene& d, const QueryArgs& Q) {
    if (hstk) hipLaunchKernelGGL((rtx_query_kernel<ANY, true, true>), grid, dim3(kBlockThreads), 0, s, d, Q);
    else if (deep) hipLaunchKernelGGL((rtx_query_kernel<ANY, true, false>), grid, dim3(kBlockThreads), 0, s, d, Q);
    else hipLaunchKernelGGL((rtx_query_kernel<ANY, false, false>), grid, dim3(kBlockThreads), 0, s, d, Q);
}

void launch_query(bool any, bool deep, bool hstk, dim3 grid, hipStream_t s, const DevScene& d, const QueryArgs& Q) {
    if (any) launch_query_t<true>(deep, hstk, grid, s, d, Q);
    else launch_query_t<false>(deep, hstk, grid, s, d, Q);
}

void launch_shade(bool deep, bool hstk, dim3 grid, hipStream_t s, const DevScene& d, const ShadeArgs& Q) {
    if (hstk) hipLaunchKernelGGL((rtx_shade_kernel<true, true>), grid, dim3(kBlockThreads), 0, s, d, Q);
    else if (deep) hipLaunchKernelGGL((rtx_shade_kernel<true, false>), grid, dim3(kBlockThreads), 0, s, d, Q);
    else hipLaunchKernelGGL((rtx_shade_kernel<false, false>), grid, dim3(kBlockThreads), 0, s, d, Q);
}

void launch_adaptive(bool deep, bool hstk, dim3 grid, hipStream_t s, const DevScene& d, const AdaptiveArgs& A) {
    if (hstk) hipLaunchKernelGGL((rtx_adaptive_kernel<true, true>), grid, dim3(kBlockThreads), 0, s, d, A);
    else if (deep) hipLaunchKernelGGL((rtx_adaptive_kernel<true, false>), grid, dim3(kBlockThreads), 0, s, d, A);
    else hipLaunchKernelGGL((rtx_adaptive_kernel<false, false>), grid, dim3(kBlockThreads), 0, s, d, A);
}

}  // namespace rtxh
