// crd_jacobian.h -- point functions of the split right-hand side f = f_D + f_R and of the Jacobian's action J(t, y) v
// (crd_jacobian.hip: crd_rhs_part_* / crd_jtimes_*), beside rhs_point_west of crd_device.h, which they leave alone.
//   f_D  the diffusion operator alone: the chain of rhs_point_west's kModelDiffusionOnly branch, so the bits of a diffusion-only
//        Goldbeter context's f
//   f_R  the kinetics alone, in rhs_point_west's own operation order: where the diffusion terms vanish exactly (a uniform field)
//        f_R has the bits of f
//   J v  the same stencil on v's activator plus the pointwise 2x2 block of the kinetics at y
// Contraction is off (crd_device.h) and every fused multiply-add is spelled out: a point's result is one fixed sequence whichever
// slab computes it.
#pragma once

#include "crd_device.h"

namespace crd {
namespace dev {

constexpr int kPartFull = CRD_PART_FULL, kPartDiffusion = CRD_PART_DIFFUSION, kPartReaction = CRD_PART_REACTION;

// du = cWn gW + (cE gE + cP d2y), dv = +0: rhs_point_west<V, kModelDiffusionOnly> with rhs_point's western term.
template <typename V>
__device__ __forceinline__ void rhs_point_diffusion(V uC, V gW, V gE, V uS, V uN, V cE, V cWn, V cP, bool zero, V &du, V &dv)
{
	const V d2y = fmadd(splat<V>(-2.0), uC, uN) + uS;
	du = fmadd(cWn, gW, fmadd(cE, gE, cP * d2y));
	dv = splat<V>(0.0);
	if (zero) du = splat<V>(0.0);
}

// w = v2(z) - v3(z, y) as rhs_point_west forms it: one quotient, numerator and denominator divided by VM3.
template <typename V>
__device__ __forceinline__ V goldbeter_w(V z, V y, typename ScalarOf<V>::type ka4)
{
	const V z2 = z * z, z4 = z2 * z2, y2 = y * y;
	const V dA = splat<V>(kGbK2 * kGbK2) + z2, dB = fmadd(splat<V>(1.0 / kGbVm3), y2, splat<V>(kGbKr * kGbKr / kGbVm3)) * fmadd(z2, z2, (V)ka4);
	return fmadd(splat<V>(kGbVm2), z2 * dB, -((y2 * z4) * dA)) * reciprocal(dA * dB);
}

// The kinetics alone.  FHN: du = u (3 - u^2) - v, dv = EPSILON u + rowp; Goldbeter: dv = w - kf y, du = rowp - dv - k z;
// diffusion-only Goldbeter: zeros.
template <typename V, int MODEL>
__device__ __forceinline__ void rhs_point_reaction(V uC, V v, typename ScalarOf<V>::type rowp, typename ScalarOf<V>::type ka4, bool zero, V &du, V &dv)
{
	if (MODEL == kModelDiffusionOnly) {
		du = dv = splat<V>(0.0);
		return;
	} else if (MODEL == CRD_MODEL_FHN) {
		du = fmadd(uC, fmadd(-uC, uC, splat<V>(3.0)), -v);
		dv = fmadd(splat<V>(kFhnEpsilon), uC, (V)rowp);
	} else {
		dv = fmadd(splat<V>(-kGbKf), v, goldbeter_w(uC, v, ka4));
		du = fmadd(splat<V>(-kGbK), uC, (V)rowp - dv);
	}
	if (zero) {
		du = splat<V>(0.0);
		dv = splat<V>(0.0);
	}
}

// The 2x2 block a = d(f_R) / d(u, v) at the state (u, v).
//   FHN        [[3 - 3 u^2, -1], [EPSILON, 0]]
//   Goldbeter  [[-w_z - k, -w_y + kf], [w_z, w_y - kf]] with (constants of src/GoldbeterModel_torus.cpp:67-78)
//     w_z = 2 z (VM2 K2^2 / (K2^2 + z^2)^2  -  2 VM3 KA^4  y^2 / (KR^2 + y^2)  z^2 / (KA^4 + z^4)^2)
//     w_y = -2 VM3 KR^2  y  z^4 / (KA^4 + z^4)  / (KR^2 + y^2)^2
//   the three denominators inverted by reciprocal(): they are sums of positive terms, at least K2^2, KR^2 and KA^4.
template <typename V, int MODEL>
__device__ __forceinline__ void jac_block(V u, V v, typename ScalarOf<V>::type ka4, V &a11, V &a12, V &a21, V &a22)
{
	if (MODEL == CRD_MODEL_FHN) {
		a11 = fmadd(splat<V>(-3.0) * u, u, splat<V>(3.0));
		a12 = splat<V>(-1.0);
		a21 = splat<V>(kFhnEpsilon);
		a22 = splat<V>(0.0);
	} else {
		const V z2 = u * u, z4 = z2 * z2, y2 = v * v;
		const V rA = reciprocal(splat<V>(kGbK2 * kGbK2) + z2), rC = reciprocal(splat<V>(kGbKr * kGbKr) + y2), rD = reciprocal(fmadd(z2, z2, (V)ka4));
		const V t2 = (splat<V>(kGbVm2 * kGbK2 * kGbK2) * rA) * rA;
		const V q3 = ((y2 * rC) * (z2 * rD)) * rD;
		const V w_z = (splat<V>(2.0) * u) * fmadd(splat<V>(-2.0 * kGbVm3) * (V)ka4, q3, t2);
		const V w_y = (splat<V>(-2.0 * kGbVm3 * kGbKr * kGbKr) * v) * ((z4 * rD) * (rC * rC));
		a11 = -w_z - splat<V>(kGbK);
		a12 = splat<V>(kGbKf) - w_y;
		a21 = w_z;
		a22 = w_y - splat<V>(kGbKf);
	}
}

// (J v) at one point: y = (yu, yv) the state, (du, dv) = v's own pair, gW / gE / dS / dN the first differences and phi neighbours of
// v's activator.  FULL is one chain: a12 dv innermost, the three diffusion terms around it, a11 du last (the order of FHN's f).
// PART: kPartFull or kPartReaction -- the diffusion part is linear, J_D v = f_D(v): rhs_point_diffusion on v.
template <typename V, int MODEL, int PART>
__device__ __forceinline__ void jac_point(V yu, V yv, V du, V dv, V gW, V gE, V dS, V dN, V cE, V cWn, V cP, typename ScalarOf<V>::type ka4, bool zero,
                                          V &ju, V &jv)
{
	static_assert(MODEL == CRD_MODEL_FHN || MODEL == CRD_MODEL_GOLDBETER, "the diffusion-only model has no block");
	static_assert(PART == kPartFull || PART == kPartReaction, "J_D v is rhs_point_diffusion on v");
	V a11, a12, a21, a22;
	jac_block<V, MODEL>(yu, yv, ka4, a11, a12, a21, a22);
	V r = (MODEL == CRD_MODEL_FHN) ? -dv : a12 * dv;
	if (PART == kPartFull) {
		const V d2y = fmadd(splat<V>(-2.0), du, dN) + dS;
		r = fmadd(cWn, gW, fmadd(cE, gE, fmadd(cP, d2y, r)));
	}
	ju = fmadd(a11, du, r);
	jv = (MODEL == CRD_MODEL_FHN) ? a21 * du : fmadd(a21, du, a22 * dv);
	if (zero) {
		ju = splat<V>(0.0);
		jv = splat<V>(0.0);
	}
}

}  // namespace dev
}  // namespace crd
