// node_math.h -- what a shading node computes for ONE value: the arithmetic of the spectral leaves, the spectral expression nodes (DESIGN.md
// section 2.8), the scalar nodes (section 2.9) and the image textures' texel addressing (section 2.6), written once for the kernels of
// device/render.hip and for the host (spectral_expr.h / scalar_node.h: the .prc loader, validate_desc, light power, the fold of constants).
// Nothing here knows Blob or DevScene: the loader includes it without the device's data layout (the sanitizer driver is built that way).
// fp32, the float functions of <math.h> on both sides; double for Planck's law.  Compiled with -ffp-contract=off everywhere.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/prgpu.h"

namespace prd {

// ---- the plain leaves ---------------------------------------------------------------------------------------
// EquidistantSpectrum.inl:34-41
__host__ __device__ __forceinline__ float equidistant_lookup(const float* data, int count, float start, float delta, float wavelength)
{
	const float af	= fmaxf(0.0f, (wavelength - start) / delta);
	const int index = (int)fminf(float(count - 2), af);
	const float t	= fminf(float(count - 1), af) - index;
	return data[index] * (1 - t) + data[index + 1] * t;
}
// SpectralUpsampler.h:45-49
__host__ __device__ __forceinline__ float upsample(const float* p, float wl)
{
	const float x = (p[0] * wl + p[1]) * wl + p[2];
	return (0.5f * x) * (1.0f / sqrtf(x * x + 1.0f)) + 0.5f;
}
// Scattering::sellmeier (base/math/Scattering.h:219-242): `nc` B coefficients, then `nc` C coefficients
// (spectrum_leaf of device/render.hip keeps its own statement of it: DESIGN.md section 5)
__host__ __device__ __forceinline__ float sellmeier(const float* B, const float* C, uint32_t nc, float wl)
{
	const float lq	= wl / 1000;
	const float lq2 = lq * lq;
	float value		= 1.0f;
	for (uint32_t i = 0; i < nc; ++i)
		value += B[i] * lq2 / (lq2 - C[i]);
	return sqrtf(value);
}

// ---- spectral expression nodes ------------------------------------------------------------------------------
__host__ __device__ __forceinline__ bool spec_is_math(uint32_t kind) { return kind == PRGPU_SPEC_MUL || (kind >= PRGPU_SPEC_ADD && kind <= PRGPU_SPEC_BRIGHTNESS_CONTRAST); }
__host__ __device__ __forceinline__ bool spec_is_unary(uint32_t kind) { return kind == PRGPU_SPEC_NEG || kind == PRGPU_SPEC_ABS || kind == PRGPU_SPEC_BRIGHTNESS_CONTRAST; }
// blackbody (core/spectral/Blackbody.h:11-28): Planck's law in double, cast to float (the node multiplies by its float peak normalisation)
constexpr double PR_LIGHT_C = 299792458.0, PR_PLANCK_H = 6.62607004081e-34, PR_BOLTZMANN_KB = 1.3806485279e-23; // base/math/SIMathConstants.h:23,37,58
__host__ __device__ __forceinline__ float expr_blackbody(float lambda_nm, float temp_kelvin)
{
	const double lambda	 = (double)(lambda_nm * 1e-9f);
	const double temp	 = (double)temp_kelvin;
	const double c1		 = 2 * PR_PLANCK_H * PR_LIGHT_C * PR_LIGHT_C;
	const double c2		 = PR_PLANCK_H * PR_LIGHT_C / PR_BOLTZMANN_KB;
	const double lambda5 = lambda * (lambda * lambda) * (lambda * lambda);
	const double f		 = c2 / (lambda * temp);
	return (float)((c1 / lambda5) / expm1(f));
}
// evalTriangle (TrianglePeakNode.cpp:8-11)
__host__ __device__ __forceinline__ float expr_peak(float wl, float centre, float radius) { return fmaxf(0.0f, 1.0f - fabsf(wl - centre) / radius); }
// one value of a unary / binary / parametrised operator (SpectralMathNode.cpp:67-96,128,188-194), in the reference's operand order: a = lhs, b = rhs
__host__ __device__ __forceinline__ float expr_op(uint32_t kind, float a, float b, float p0, float p1)
{
	switch (kind) {
	case PRGPU_SPEC_MUL: return a * b;
	case PRGPU_SPEC_ADD: return a + b;
	case PRGPU_SPEC_SUB: return a - b;
	case PRGPU_SPEC_DIV: return a / b;
	case PRGPU_SPEC_NEG: return -a;
	case PRGPU_SPEC_ABS: return fabsf(a);
	case PRGPU_SPEC_MAX: return fmaxf(a, b);
	case PRGPU_SPEC_MIN: return fminf(a, b);
	case PRGPU_SPEC_BURN: return 1 - (1 - a) / (b + 1);
	case PRGPU_SPEC_SCREEN: return 1 - (1 - a) * (1 - b);
	case PRGPU_SPEC_DODGE: return a / ((1 - b) + 1);
	case PRGPU_SPEC_OVERLAY: return a * (a + 2 * b * (1 - a));
	case PRGPU_SPEC_SOFTLIGHT: {
		const float r = 1 - (1 - a) * (1 - b);
		return ((1 - a) * b + r) * a;
	}
	case PRGPU_SPEC_HARDLIGHT: {
		const float k1 = 1 - (1 - 2 * (b - 0.5f)) * (1 - a);
		const float k2 = 2 * b * a;
		return b <= 0.5f ? k2 : k1;
	}
	case PRGPU_SPEC_BLEND: return a * (1 - p0) + b * p0;
	case PRGPU_SPEC_BRIGHTNESS_CONTRAST: return fmaxf((1.0f + p1) * a + (p0 - p1 * 0.5f), 0.0f);
	default: return 0.0f;
	}
}

// ---- scalar nodes -------------------------------------------------------------------------------------------
// (scalar_run of device/render.hip keeps its own statement of these two: DESIGN.md section 5)
__host__ __device__ __forceinline__ bool scalar_is_op(uint32_t kind) { return kind >= PRGPU_SPEC_SCALAR_ADD && kind <= PRGPU_SPEC_SCALAR_COS; }
__host__ __device__ __forceinline__ bool scalar_is_unary(uint32_t kind)
{
	return scalar_is_op(kind) && kind != PRGPU_SPEC_SCALAR_ADD && kind != PRGPU_SPEC_SCALAR_SUB && kind != PRGPU_SPEC_SCALAR_MUL && kind != PRGPU_SPEC_SCALAR_DIV
		   && kind != PRGPU_SPEC_SCALAR_MAX && kind != PRGPU_SPEC_SCALAR_MIN && kind != PRGPU_SPEC_SCALAR_POW;
}
// one operator of ScalarMathNode.cpp:109-144 that has a device kind, in the reference's operand order (std::max / std::min as they compare)
__host__ __device__ __forceinline__ float scalar_op(uint32_t kind, float a, float b)
{
	switch (kind) {
	case PRGPU_SPEC_SCALAR_ADD: return a + b;
	case PRGPU_SPEC_SCALAR_SUB: return a - b;
	case PRGPU_SPEC_SCALAR_MUL: return a * b;
	case PRGPU_SPEC_SCALAR_DIV: return a / b;
	case PRGPU_SPEC_SCALAR_NEG: return -a;
	case PRGPU_SPEC_SCALAR_ABS: return fabsf(a);
	case PRGPU_SPEC_SCALAR_MAX: return a < b ? b : a;
	case PRGPU_SPEC_SCALAR_MIN: return b < a ? b : a;
	case PRGPU_SPEC_SCALAR_SQRT: return sqrtf(a);
	case PRGPU_SPEC_SCALAR_POW: return powf(a, b);
	case PRGPU_SPEC_SCALAR_FLOOR: return floorf(a);
	case PRGPU_SPEC_SCALAR_CEIL: return ceilf(a);
	case PRGPU_SPEC_SCALAR_ROUND: return roundf(a);
	case PRGPU_SPEC_SCALAR_EXP: return expf(a);
	case PRGPU_SPEC_SCALAR_LOG: return logf(a);
	case PRGPU_SPEC_SCALAR_SIN: return sinf(a);
	case PRGPU_SPEC_SCALAR_COS: return cosf(a);
	default: return 0.0f;
	}
}

// ---- image textures: texel addressing -----------------------------------------------------------------------
// One texel index of an image texture along an axis of `n` texels, wrapped by `mode` (0 black, 1 clamp, 2 periodic, 3 mirror: period 2n,
// second half reflected); -1 selects the black texel.  OpenImageIO's wrap functions (texture.h, TextureOpt::Wrap), restated.
__host__ __device__ __forceinline__ int image_wrap(int i, int n, int mode)
{
	if (mode == 1)
		return min(max(i, 0), n - 1);
	if (mode == 2) {
		const int r = i % n;
		return r < 0 ? r + n : r;
	}
	if (mode == 3) {
		int r = i % (2 * n);
		r	  = r < 0 ? r + 2 * n : r;
		return r >= n ? 2 * n - 1 - r : r;
	}
	return (i < 0 || i >= n) ? -1 : i;
}
// a texel coordinate as an integer the wraps can take: floor, held inside +-2^30 (a NaN ends at the lower bound)
__host__ __device__ __forceinline__ int image_floor(float x) { return (int)fminf(fmaxf(floorf(x), -1073741824.0f), 1073741824.0f); }

} // namespace prd
