// node_program.h -- the postfix program of a tree of operator nodes, as the device's two stack machines run it (expr_eval and scalar_run of
// device/render.hip; DESIGN.md sections 2.8 and 2.9): one word per node reached, a shared node once per path to it; the operand that needs
// the deeper stack goes first, and bit 31 of an operator's word says that this was its RIGHT operand.  Sizing and emission are written here
// once; a family of nodes (spectral_expr.h, scalar_node.h) brings its two kind predicates and keeps its own flags on top of the extent.
#pragma once
#include "../../../include/prgpu.h"
#include <algorithm>
#include <cstdint>
#include <vector>

namespace prgpu_host {
struct NodeFamily {
	bool (*is_op)(uint32_t kind);	 // an operator: lhs (and rhs) name operands that precede the node; every other kind is a leaf of a program
	bool (*is_unary)(uint32_t kind); // an operator that reads lhs alone
};
// The operand stack a node's program needs (leaf 1; binary: the larger of the operands', one more on a tie) and the program's length
// (saturating at 2^20: op(x, x) doubles it per level).
struct ProgramExtent {
	uint32_t need = 1, length = 1;
};
// the operands' entries of `info` (`b` null for a unary operator); false for a leaf, and for an operand beyond `info` (refused by the caller)
template <class Info>
bool program_operands(const NodeFamily& f, const prgpu_spectrum& n, const std::vector<Info>& info, const Info*& a, const Info*& b)
{
	if (!f.is_op(n.kind))
		return false;
	const bool unary = f.is_unary(n.kind);
	if (n.lhs >= info.size() || (!unary && n.rhs >= info.size()))
		return false;
	a = &info[n.lhs];
	b = unary ? nullptr : &info[n.rhs];
	return true;
}
inline ProgramExtent program_extent(const ProgramExtent& a, const ProgramExtent* b)
{
	ProgramExtent r;
	r.need	 = !b ? a.need : a.need == b->need ? a.need + 1u : std::max(a.need, b->need);
	r.length = std::min<uint32_t>(a.length + (b ? b->length : 0u) + 1u, 1u << 20);
	return r;
}
template <class Info>
void program_emit(const NodeFamily& f, const prgpu_spectrum* spectra, const std::vector<Info>& info, uint32_t id, std::vector<uint32_t>& out)
{
	const prgpu_spectrum& n = spectra[id];
	uint32_t word			= id;
	if (f.is_op(n.kind)) {
		const bool unary = f.is_unary(n.kind);
		const bool swap	 = !unary && info[n.rhs].need > info[n.lhs].need;
		program_emit(f, spectra, info, swap ? n.rhs : n.lhs, out);
		if (!unary)
			program_emit(f, spectra, info, swap ? n.lhs : n.rhs, out);
		word |= swap ? 0x80000000u : 0u;
	}
	out.push_back(word);
}
// "operands must precede the node": what keeps the node array acyclic and lets one pass size every node from its operands
inline bool program_operands_precede(const NodeFamily& f, const prgpu_spectrum& n, uint32_t i) { return n.lhs < i && (f.is_unary(n.kind) || n.rhs < i); }
} // namespace prgpu_host
