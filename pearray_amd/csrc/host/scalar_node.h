// scalar_node.h -- the host's half of the scalar nodes (include/prgpu.h, PRGPU_SPEC_SCALAR_IMAGE .. PRGPU_SPEC_SCALAR_COS and the
// PRGPU_MATF_NODE_* bits): what the .prc loader, validate_desc and the compile to postfix programs share.
// Header only, like spectral_expr.h: the loader is also built without setup.cpp (the sanitizer driver).  The operators that have a device
// kind are the device's own text (device/node_math.h, scalar_op); the names that only fold on the host restate ScalarMathNode.cpp here
// (fp32, the std:: float overloads).  The program format is node_program.h's.
#pragma once
#include "../../../include/prgpu.h"
#include "../device/node_math.h"
#include "node_program.h"
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace prgpu_host {
using prd::scalar_is_op;
using prd::scalar_is_unary;
inline bool scalar_is_kind(uint32_t kind) { return kind == PRGPU_SPEC_SCALAR_IMAGE || scalar_is_op(kind); }
constexpr NodeFamily SCALAR_FAMILY = { scalar_is_op, scalar_is_unary };

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
// FloatScalarNode::eval of a math node over constants (ScalarMathNode.cpp:109-144), by name: every name folds -- a name that has a device
// kind by the device's scalar_op, the others here
inline float scalar_fold(const std::string& name, float a, float b)
{
	const ScalarOpName* op = scalar_op_by_name(name);
	if (op && op->kind != 0)
		return prd::scalar_op(op->kind, a, b);
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
	if (name == "cbrt") return std::cbrt(a);
	if (name == "atan2") return std::atan2(a, b);
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

// the extent of a scalar node's program (node_program.h) from its operands' (which precede it), as ExprInfo has it for the spectral nodes
struct ScalarInfo : ProgramExtent {
	bool textured = false; // a SCALAR_IMAGE somewhere below
};
inline ScalarInfo scalar_info_of(const prgpu_spectrum& n, const std::vector<ScalarInfo>& info)
{
	ScalarInfo r;
	r.textured = n.kind == PRGPU_SPEC_SCALAR_IMAGE;
	const ScalarInfo *a, *b;
	if (!program_operands(SCALAR_FAMILY, n, info, a, b))
		return r;
	static_cast<ProgramExtent&>(r) = program_extent(*a, b);
	r.textured					   = a->textured || (b && b->textured);
	return r;
}
// postfix program of the scalar tree rooted at `id`, for scalar_run of device/render.hip
inline void scalar_emit(const prgpu_spectrum* spectra, const std::vector<ScalarInfo>& info, uint32_t id, std::vector<uint32_t>& out) { program_emit(SCALAR_FAMILY, spectra, info, id, out); }
} // namespace prgpu_host
