// spectral_expr.h -- the host's half of the spectral expression nodes (include/prgpu.h, PRGPU_SPEC_ADD .. PRGPU_SPEC_PEAK):
// what the .prc loader, validate_desc, the host evaluator (light power, the spd histogram) and the compile to postfix programs share.
// Header only: the loader is also built without setup.cpp (the sanitizer driver).  The arithmetic is the device's own text
// (device/node_math.h: expr_op, expr_blackbody, expr_peak and the plain leaves' primitives); the program format is node_program.h's.
#pragma once
#include "../../../include/prgpu.h"
#include "../device/node_math.h"
#include "node_program.h"
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace prgpu_host {
using prd::spec_is_math;
using prd::spec_is_unary;
inline bool spec_is_uv(uint32_t kind) { return kind == PRGPU_SPEC_CHECKER || kind == PRGPU_SPEC_IMAGE; }
constexpr NodeFamily SPEC_FAMILY = { spec_is_math, spec_is_unary };

// normFactor (BlackbodyNode.cpp:8-14): the peak normalisation a constant temperature always gets (:106-109)
inline float blackbody_norm(float temp_kelvin)
{
	const float max_nm	= 2.897771955e+6f / temp_kelvin;
	const float max_val = prd::expr_blackbody(max_nm, temp_kelvin);
	return 1 / max_val;
}
// FloatSpectralNode::eval of a plain leaf at one wavelength, over the table array `tables`: spectrum_leaf of device/render.hip, from the
// same primitives (an image texture, which depends on uv, is none of these)
inline float spectrum_leaf_at(const prgpu_spectrum& n, const float* tables, float wl)
{
	switch (n.kind) {
	case PRGPU_SPEC_CONST: return n.p[0];
	case PRGPU_SPEC_PARAMETRIC: return prd::upsample(n.p, wl);
	case PRGPU_SPEC_PARAMETRIC_SCALED: return prd::upsample(n.p, wl) * n.p[3];
	case PRGPU_SPEC_TABLE: return prd::equidistant_lookup(tables + n.table_offset, (int)n.table_count, n.wl_start, (n.wl_end - n.wl_start) / (n.table_count - 1), wl);
	case PRGPU_SPEC_SELLMEIER: {
		const uint32_t nc = n.table_count / 2;
		const float* B	  = tables + n.table_offset;
		return prd::sellmeier(B, B + nc, nc, wl);
	}
	default: return 0.0f;
	}
}
// FloatSpectralNode::eval of any node that does not depend on uv, at one wavelength; `leaf` evaluates the kinds CONST .. TABLE and SELLMEIER
// (spectrum_leaf_at over the caller's tables).
// (validate_desc bounds an expression's size; the depth guard covers arrays that were not validated)
template <class Leaf>
float expr_eval_at(const prgpu_spectrum* spectra, uint32_t n_spectra, uint32_t id, float wl, Leaf&& leaf, int depth = 0)
{
	if (id >= n_spectra || depth > 2 * PRGPU_EXPR_MAX_PROGRAM)
		return 0.0f;
	const prgpu_spectrum& n = spectra[id];
	if (n.kind == PRGPU_SPEC_BLACKBODY)
		return prd::expr_blackbody(wl, n.p[0]) * n.p[1];
	if (n.kind == PRGPU_SPEC_PEAK)
		return prd::expr_peak(wl, n.p[0], n.p[1]);
	if (!spec_is_math(n.kind))
		return leaf(n, wl);
	const float a = expr_eval_at(spectra, n_spectra, n.lhs, wl, leaf, depth + 1);
	const float b = spec_is_unary(n.kind) ? 0.0f : expr_eval_at(spectra, n_spectra, n.rhs, wl, leaf, depth + 1);
	return prd::expr_op(n.kind, a, b, n.p[0], n.p[1]);
}

// What the compile needs to know of a node, from its operands' (which precede it): the extent of its program (node_program.h) and three flags.
struct ExprInfo : ProgramExtent {
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
	const ExprInfo *a, *b;
	if (!program_operands(SPEC_FAMILY, n, info, a, b))
		return r;
	static_cast<ProgramExtent&>(r) = program_extent(*a, b);
	r.varying					   = a->varying || (b && b->varying);
	r.sellmeier					   = a->sellmeier || (b && b->sellmeier);
	r.expression = !b || n.kind != PRGPU_SPEC_MUL || a->expression || b->expression || a->varying || b->varying || spectra[n.lhs].kind == PRGPU_SPEC_MUL || spectra[n.rhs].kind == PRGPU_SPEC_MUL;
	return r;
}
// postfix program of the expression rooted at `id`, for expr_eval of device/render.hip
inline void expr_emit(const prgpu_spectrum* spectra, const std::vector<ExprInfo>& info, uint32_t id, std::vector<uint32_t>& out) { program_emit(SPEC_FAMILY, spectra, info, id, out); }
} // namespace prgpu_host
