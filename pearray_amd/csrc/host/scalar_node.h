// scalar_node.h -- the host's half of the scalar nodes (include/prgpu.h, PRGPU_SPEC_SCALAR_IMAGE .. PRGPU_SPEC_SCALAR_COS and the
// PRGPU_MATF_NODE_* bits): what the .prc loader, validate_desc and the compile to postfix programs share.
// Header only, like spectral_expr.h: the loader is also built without setup.cpp (the sanitizer driver).  The arithmetic restates
// ScalarMathNode.cpp (fp32, the std:: float overloads); scalar_op of device/render.hip restates the device's share of it.
#pragma once
#include "../../../include/prgpu.h"
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace prgpu_host {
inline bool scalar_is_op(uint32_t kind) { return kind >= PRGPU_SPEC_SCALAR_ADD && kind <= PRGPU_SPEC_SCALAR_COS; }
inline bool scalar_is_kind(uint32_t kind) { return kind == PRGPU_SPEC_SCALAR_IMAGE || scalar_is_op(kind); }
inline bool scalar_is_unary(uint32_t kind)
{
	return scalar_is_op(kind) && kind != PRGPU_SPEC_SCALAR_ADD && kind != PRGPU_SPEC_SCALAR_SUB && kind != PRGPU_SPEC_SCALAR_MUL && kind != PRGPU_SPEC_SCALAR_DIV
		   && kind != PRGPU_SPEC_SCALAR_MAX && kind != PRGPU_SPEC_SCALAR_MIN && kind != PRGPU_SPEC_SCALAR_POW;
}

// The 32 names ScalarMathPlugin registers (ScalarMathNode.cpp:219-228) and `pow`, whose class the file defines (:144) without registering
// it: accepted here.  `kind` is the device enumerator, or 0 for a name that only folds on the host.
struct ScalarOpName {
	const char* name;
	uint32_t kind;
	int arity;
};
inline const ScalarOpName* scalar_op_by_name(const std::string& name)
{
	static const ScalarOpName ops[] = {
		{ "add", PRGPU_SPEC_SCALAR_ADD, 2 }, { "sub", PRGPU_SPEC_SCALAR_SUB, 2 }, { "subtract", PRGPU_SPEC_SCALAR_SUB, 2 }, { "mul", PRGPU_SPEC_SCALAR_MUL, 2 },
		{ "multiply", PRGPU_SPEC_SCALAR_MUL, 2 }, { "div", PRGPU_SPEC_SCALAR_DIV, 2 }, { "divide", PRGPU_SPEC_SCALAR_DIV, 2 }, { "neg", PRGPU_SPEC_SCALAR_NEG, 1 },
		{ "negate", PRGPU_SPEC_SCALAR_NEG, 1 }, { "sin", PRGPU_SPEC_SCALAR_SIN, 1 }, { "cos", PRGPU_SPEC_SCALAR_COS, 1 }, { "tan", 0, 1 }, { "asin", 0, 1 },
		{ "acos", 0, 1 }, { "atan", 0, 1 }, { "sinh", 0, 1 }, { "cosh", 0, 1 }, { "tanh", 0, 1 }, { "asinh", 0, 1 }, { "acosh", 0, 1 }, { "atanh", 0, 1 },
		{ "exp", PRGPU_SPEC_SCALAR_EXP, 1 }, { "log", PRGPU_SPEC_SCALAR_LOG, 1 }, { "abs", PRGPU_SPEC_SCALAR_ABS, 1 }, { "sqrt", PRGPU_SPEC_SCALAR_SQRT, 1 },
		{ "cbrt", 0, 1 }, { "ceil", PRGPU_SPEC_SCALAR_CEIL, 1 }, { "floor", PRGPU_SPEC_SCALAR_FLOOR, 1 }, { "round", PRGPU_SPEC_SCALAR_ROUND, 1 },
		{ "atan2", 0, 2 }, { "max", PRGPU_SPEC_SCALAR_MAX, 2 }, { "min", PRGPU_SPEC_SCALAR_MIN, 2 }, { "pow", PRGPU_SPEC_SCALAR_POW, 2 },
	};
	for (const ScalarOpName& op : ops)
		if (name == op.name)
			return &op;
	return nullptr;
}
// FloatScalarNode::eval of a math node over constants (ScalarMathNode.cpp:109-144), by name: every name folds
inline float scalar_fold(const std::string& name, float a, float b)
{
	if (name == "add") return a + b;
	if (name == "sub" || name == "subtract") return a - b;
	if (name == "mul" || name == "multiply") return a * b;
	if (name == "div" || name == "divide") return a / b;
	if (name == "neg" || name == "negate") return -a;
	if (name == "sin") return std::sin(a);
	if (name == "cos") return std::cos(a);
	if (name == "tan") return std::tan(a);
	if (name == "asin") return std::asin(a);
	if (name == "acos") return std::acos(a);
	if (name == "atan") return std::atan(a);
	if (name == "sinh") return std::sinh(a);
	if (name == "cosh") return std::cosh(a);
	if (name == "tanh") return std::tanh(a);
	if (name == "asinh") return std::asinh(a);
	if (name == "acosh") return std::acosh(a);
	if (name == "atanh") return std::atanh(a);
	if (name == "exp") return std::exp(a);
	if (name == "log") return std::log(a);
	if (name == "abs") return std::abs(a);
	if (name == "sqrt") return std::sqrt(a);
	if (name == "cbrt") return std::cbrt(a);
	if (name == "ceil") return std::ceil(a);
	if (name == "floor") return std::floor(a);
	if (name == "round") return std::round(a);
	if (name == "atan2") return std::atan2(a, b);
	if (name == "max") return std::max(a, b);
	if (name == "min") return std::min(a, b);
	if (name == "pow") return std::pow(a, b);
	return 0.0f;
}

// The float fields of a material a scalar node may be bound to, in the order of their PRGPU_MATF_NODE_* bits: roughness_x, roughness_y,
// principled[0 .. 9].
constexpr int SCALAR_SLOTS = 2 + PRGPU_PRINCIPLED_COUNT;
inline uint32_t scalar_slot_bit(int slot) { return PRGPU_MATF_NODE_ROUGHNESS_X << slot; }
inline float& scalar_slot_field(prgpu_material& m, int slot) { return slot == 0 ? m.roughness_x : slot == 1 ? m.roughness_y : m.principled[slot - 2]; }
inline float scalar_slot_field(const prgpu_material& m, int slot) { return slot == 0 ? m.roughness_x : slot == 1 ? m.roughness_y : m.principled[slot - 2]; }
// the slots a kind reads (a bit elsewhere is refused)
inline bool scalar_slot_of_kind(uint32_t mat_kind, int slot)
{
	if (mat_kind == PRGPU_MAT_ROUGH_CONDUCTOR || mat_kind == PRGPU_MAT_ROUGH_DIELECTRIC)
		return slot < 2;
	if (mat_kind == PRGPU_MAT_OREN_NAYAR)
		return slot == 0;
	if (mat_kind == PRGPU_MAT_PRINCIPLED)
		return slot != 1;
	return false;
}
// the node index a bound field holds, or PRGPU_INVALID_ID when the float is no index of the array
inline uint32_t scalar_slot_node(float field, uint32_t n_spectra)
{
	if (!(field >= 0.0f) || !(field < 16777216.0f) || field != std::floor(field) || uint32_t(field) >= n_spectra)
		return PRGPU_INVALID_ID;
	return uint32_t(field);
}

// operand stack and program length of a scalar node from its operands' (which precede it), as ExprInfo has them for the spectral nodes
struct ScalarInfo {
	uint32_t need = 1, length = 1;
	bool textured = false; // a SCALAR_IMAGE somewhere below
};
inline ScalarInfo scalar_info_of(const prgpu_spectrum& n, const std::vector<ScalarInfo>& info)
{
	ScalarInfo r;
	r.textured = n.kind == PRGPU_SPEC_SCALAR_IMAGE;
	if (!scalar_is_op(n.kind))
		return r;
	const bool unary = scalar_is_unary(n.kind);
	if (n.lhs >= info.size() || (!unary && n.rhs >= info.size())) // (refused by the caller)
		return r;
	const ScalarInfo& a = info[n.lhs];
	if (unary) {
		r		 = a;
		r.length = std::min<uint32_t>(a.length + 1u, 1u << 20);
		return r;
	}
	const ScalarInfo& b = info[n.rhs];
	r.need				= a.need == b.need ? a.need + 1u : std::max(a.need, b.need);
	r.length			= std::min<uint32_t>(a.length + b.length + 1u, 1u << 20);
	r.textured			= a.textured || b.textured;
	return r;
}
// postfix program of the scalar tree rooted at `id` (device/render.hip, scalar_run): the words of expr_emit -- a node index, bit 31 when the
// right operand went first (the one that needs the deeper stack does)
inline void scalar_emit(const prgpu_spectrum* spectra, const std::vector<ScalarInfo>& info, uint32_t id, std::vector<uint32_t>& out)
{
	const prgpu_spectrum& n = spectra[id];
	if (!scalar_is_op(n.kind)) {
		out.push_back(id);
		return;
	}
	if (scalar_is_unary(n.kind)) {
		scalar_emit(spectra, info, n.lhs, out);
		out.push_back(id);
		return;
	}
	const bool swap = info[n.rhs].need > info[n.lhs].need;
	scalar_emit(spectra, info, swap ? n.rhs : n.lhs, out);
	scalar_emit(spectra, info, swap ? n.lhs : n.rhs, out);
	out.push_back(id | (swap ? 0x80000000u : 0u));
}
} // namespace prgpu_host
