// spectral_expr.h -- the host's half of the spectral expression nodes (include/prgpu.h, PRGPU_SPEC_ADD .. PRGPU_SPEC_PEAK):
// what the .prc loader, validate_desc, the host evaluator (light power, the spd histogram) and the compile to postfix programs share.
// Header only: the loader is also built without setup.cpp (the sanitizer driver).  The arithmetic restates expr_op / expr_leaf of
// device/render.hip statement by statement (fp32; double for Planck's law).
#pragma once
#include "../../../include/prgpu.h"
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace prgpu_host {
inline bool spec_is_math(uint32_t kind) { return kind == PRGPU_SPEC_MUL || (kind >= PRGPU_SPEC_ADD && kind <= PRGPU_SPEC_BRIGHTNESS_CONTRAST); }
inline bool spec_is_unary(uint32_t kind) { return kind == PRGPU_SPEC_NEG || kind == PRGPU_SPEC_ABS || kind == PRGPU_SPEC_BRIGHTNESS_CONTRAST; }
inline bool spec_is_uv(uint32_t kind) { return kind == PRGPU_SPEC_CHECKER || kind == PRGPU_SPEC_IMAGE; }

// blackbody (core/spectral/Blackbody.h:11-28) with the constants of base/math/SIMathConstants.h:23,37,58
inline float blackbody(float lambda_nm, float temp_kelvin)
{
	const double c = 299792458.0, h = 6.62607004081e-34, kb = 1.3806485279e-23;
	const double lambda	 = (double)(lambda_nm * 1e-9f);
	const double temp	 = (double)temp_kelvin;
	const double c1		 = 2 * h * c * c;
	const double c2		 = h * c / kb;
	const double lambda5 = lambda * (lambda * lambda) * (lambda * lambda);
	const double f		 = c2 / (lambda * temp);
	return (float)((c1 / lambda5) / std::expm1(f));
}
// normFactor (BlackbodyNode.cpp:8-14): the peak normalisation a constant temperature always gets (:106-109)
inline float blackbody_norm(float temp_kelvin)
{
	const float max_nm	= 2.897771955e+6f / temp_kelvin;
	const float max_val = blackbody(max_nm, temp_kelvin);
	return 1 / max_val;
}
// one wavelength of an operator (SpectralMathNode.cpp:67-96,128,188-194), a = lhs, b = rhs
inline float expr_op(uint32_t kind, float a, float b, float p0, float p1)
{
	switch (kind) {
	case PRGPU_SPEC_MUL: return a * b;
	case PRGPU_SPEC_ADD: return a + b;
	case PRGPU_SPEC_SUB: return a - b;
	case PRGPU_SPEC_DIV: return a / b;
	case PRGPU_SPEC_NEG: return -a;
	case PRGPU_SPEC_ABS: return std::fabs(a);
	case PRGPU_SPEC_MAX: return std::fmax(a, b);
	case PRGPU_SPEC_MIN: return std::fmin(a, b);
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
	case PRGPU_SPEC_BRIGHTNESS_CONTRAST: return std::fmax((1.0f + p1) * a + (p0 - p1 * 0.5f), 0.0f);
	default: return 0.0f;
	}
}
// FloatSpectralNode::eval of any node that does not depend on uv, at one wavelength; `leaf` evaluates the kinds CONST .. TABLE and SELLMEIER.
// (validate_desc bounds an expression's size; the depth guard covers arrays that were not validated)
template <class Leaf>
float expr_eval_at(const prgpu_spectrum* spectra, uint32_t n_spectra, uint32_t id, float wl, Leaf&& leaf, int depth = 0)
{
	if (id >= n_spectra || depth > 2 * PRGPU_EXPR_MAX_PROGRAM)
		return 0.0f;
	const prgpu_spectrum& n = spectra[id];
	if (n.kind == PRGPU_SPEC_BLACKBODY)
		return blackbody(wl, n.p[0]) * n.p[1];
	if (n.kind == PRGPU_SPEC_PEAK)
		return std::fmax(0.0f, 1.0f - std::fabs(wl - n.p[0]) / n.p[1]);
	if (!spec_is_math(n.kind))
		return leaf(n, wl);
	const float a = expr_eval_at(spectra, n_spectra, n.lhs, wl, leaf, depth + 1);
	const float b = spec_is_unary(n.kind) ? 0.0f : expr_eval_at(spectra, n_spectra, n.rhs, wl, leaf, depth + 1);
	return expr_op(n.kind, a, b, n.p[0], n.p[1]);
}

// What the compile needs to know of a node, from its operands' (which precede it): the operand stack its program needs when the deeper
// operand is emitted first (leaf 1; binary: max, one more on a tie), the program's length (saturating), and three flags.
struct ExprInfo {
	uint32_t need = 1, length = 1;
	bool varying	= false; // NodeFlag::SpectralVarying: SELLMEIER, BLACKBODY, PEAK, or a math node over one
	bool sellmeier	= false; // a refractive-index node somewhere below (not a radiance)
	bool expression = false; // evaluated by a program where a root names it (everything but a plain leaf and a MUL of two plain leaves)
};
inline ExprInfo expr_info_of(const prgpu_spectrum& n, const std::vector<ExprInfo>& info, const prgpu_spectrum* spectra)
{
	ExprInfo r;
	r.sellmeier	 = n.kind == PRGPU_SPEC_SELLMEIER;
	r.varying	 = r.sellmeier || n.kind == PRGPU_SPEC_BLACKBODY || n.kind == PRGPU_SPEC_PEAK;
	r.expression = n.kind > PRGPU_SPEC_IMAGE && n.kind <= PRGPU_SPEC_PEAK; // (the scalar kinds beyond are no spectra: scalar_node.h)
	if (!spec_is_math(n.kind))
		return r;
	const bool unary = spec_is_unary(n.kind);
	if (n.lhs >= info.size() || (!unary && n.rhs >= info.size())) // (refused by the caller)
		return r;
	const ExprInfo& a = info[n.lhs];
	if (unary) {
		r			 = a;
		r.length	 = std::min<uint32_t>(a.length + 1u, 1u << 20);
		r.expression = true;
		return r;
	}
	const ExprInfo& b = info[n.rhs];
	r.need			  = a.need == b.need ? a.need + 1u : std::max(a.need, b.need);
	r.length		  = std::min<uint32_t>(a.length + b.length + 1u, 1u << 20);
	r.varying		  = a.varying || b.varying;
	r.sellmeier		  = a.sellmeier || b.sellmeier;
	r.expression	  = n.kind != PRGPU_SPEC_MUL || a.expression || b.expression || a.varying || b.varying || spectra[n.lhs].kind == PRGPU_SPEC_MUL || spectra[n.rhs].kind == PRGPU_SPEC_MUL;
	return r;
}
// postfix program of the expression rooted at `id` (device/render.hip, expr_eval): a word per node, the operand that needs the deeper stack
// first; bit 31 tells the operator that its right operand went first
inline void expr_emit(const prgpu_spectrum* spectra, const std::vector<ExprInfo>& info, uint32_t id, std::vector<uint32_t>& out)
{
	const prgpu_spectrum& n = spectra[id];
	if (!spec_is_math(n.kind)) {
		out.push_back(id);
		return;
	}
	if (spec_is_unary(n.kind)) {
		expr_emit(spectra, info, n.lhs, out);
		out.push_back(id);
		return;
	}
	const bool swap = info[n.rhs].need > info[n.lhs].need;
	expr_emit(spectra, info, swap ? n.rhs : n.lhs, out);
	expr_emit(spectra, info, swap ? n.lhs : n.rhs, out);
	out.push_back(id | (swap ? 0x80000000u : 0u));
}
} // namespace prgpu_host
