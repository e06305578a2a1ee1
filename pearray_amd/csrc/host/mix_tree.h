// mix_tree.h -- the host's half of nested BLEND / ADD materials (include/prgpu.h, PRGPU_MIX_MAX_DEPTH / _LEAVES): what
// the .prc loader, validate_desc, prgpu_mix_leaves and the upload of a scene share.  The tree below a combinator is compiled away here:
// IMaterial::eval of a blend / add is linear in the plain leaves it reaches (blend.cpp:41-75, add.cpp:40-66), so a vertex walks one table
// row of (leaf, weight coefficient, pdf coefficient) instead of the tree.  Header only: the loader is also built without setup.cpp (the
// sanitizer driver).
#pragma once
#include "../../../include/prgpu.h"
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace prgpu_host {
inline bool mat_is_combinator(uint32_t kind) { return kind == PRGPU_MAT_BLEND || kind == PRGPU_MAT_ADD; }
// IMaterial::hasOnlyDeltaDistribution of a plain kind (device/render.hip, mix_delta_only)
inline bool mat_plain_delta_only(uint32_t kind) { return kind == PRGPU_MAT_DIELECTRIC || kind == PRGPU_MAT_CONDUCTOR || kind == PRGPU_MAT_MIRROR || kind == PRGPU_MAT_NULL; }

// Size of the tree below every material, from its children's (which precede it): combinators on the longest path down, leaves with a
// shared child counted once per path.  A plain material is (0, 1).  Saturating: a chain of shared children doubles the leaves per level.
struct MixExtent {
	uint32_t depth = 0, leaves = 1;
};
inline MixExtent mix_extent_of(const MixExtent& a, const MixExtent& b)
{
	MixExtent r;
	r.depth	 = std::max(a.depth, b.depth) + 1u;
	r.leaves = std::min<uint32_t>(a.leaves + b.leaves, 1u << 20);
	return r;
}
// the refusal both bounds share, or "" (`what`: "blend material 7", "material 'coat'")
inline std::string mix_extent_refusal(const MixExtent& e, const std::string& what)
{
	if (e.depth > PRGPU_MIX_MAX_DEPTH)
		return what + ": " + std::to_string(e.depth) + " blend / add materials on a path to a leaf, more than PRGPU_MIX_MAX_DEPTH (" + std::to_string(PRGPU_MIX_MAX_DEPTH) + ")";
	if (e.leaves > PRGPU_MIX_MAX_LEAVES)
		return what + ": " + (e.leaves >= (1u << 20) ? std::string("too many") : std::to_string(e.leaves)) + " leaves below it, more than PRGPU_MIX_MAX_LEAVES (" + std::to_string(PRGPU_MIX_MAX_LEAVES) + ")";
	return std::string();
}
// extents of a whole material array whose combinators name earlier materials (entries with a bad child keep (0, 1): refused by the caller)
inline std::vector<MixExtent> mix_extents(const prgpu_material* mats, uint32_t n)
{
	std::vector<MixExtent> e(n);
	for (uint32_t i = 0; i < n; ++i)
		if (mat_is_combinator(mats[i].kind) && mats[i].two_sided < i && mats[i].thin < i)
			e[i] = mix_extent_of(e[mats[i].two_sided], e[mats[i].thin]);
	return e;
}
// `pred(material)` of any leaf below `id`, every leaf a sample can pick included (a validated array: children precede, bounded depth)
template <class Pred>
bool mix_any_leaf(const prgpu_material* mats, uint32_t id, Pred&& pred, int depth = 0)
{
	const prgpu_material& m = mats[id];
	if (!mat_is_combinator(m.kind) || depth > PRGPU_MIX_MAX_DEPTH)
		return !mat_is_combinator(m.kind) && pred(m);
	return mix_any_leaf(mats, m.two_sided, pred, depth + 1) || mix_any_leaf(mats, m.thin, pred, depth + 1);
}

// One root, flattened: what a table row holds and prgpu_mix_leaves returns.
struct MixRow {
	std::vector<prgpu_mix_leaf> leaves; // the leaves eval reaches, depth first, child 1 before child 2
	bool delta_only		 = false;
	uint32_t symbol_leaf = PRGPU_INVALID_ID, flag_leaf = PRGPU_INVALID_ID; // indices into `leaves`
};
// hasOnlyDeltaDistribution, recursively: a combinator has it exactly when both children have it (blend.cpp:156-173, add.cpp:141-158)
inline bool mix_delta_only(const prgpu_material* mats, uint32_t id, int depth = 0)
{
	const prgpu_material& m = mats[id];
	if (!mat_is_combinator(m.kind) || depth > PRGPU_MIX_MAX_DEPTH)
		return mat_plain_delta_only(m.kind);
	return mix_delta_only(mats, m.two_sided, depth + 1) && mix_delta_only(mats, m.thin, depth + 1);
}
// eval below `id`, whose weight carries `a` and whose pdf carries `b` so far.  symbol / flag: this subtree is where the root's scattering
// type resp. delta flag comes from (flag: every form from the root down to here was one-sided).
inline void mix_flatten_into(const prgpu_material* mats, uint32_t id, float a, float b, bool symbol, bool flag, MixRow& row, int depth = 0)
{
	const prgpu_material& m = mats[id];
	if (!mat_is_combinator(m.kind) || depth > PRGPU_MIX_MAX_DEPTH) {
		if (symbol)
			row.symbol_leaf = (uint32_t)row.leaves.size();
		if (flag)
			row.flag_leaf = (uint32_t)row.leaves.size();
		row.leaves.push_back(prgpu_mix_leaf{ id, a, b });
		return;
	}
	const bool add	= m.kind == PRGPU_MAT_ADD;
	const float f	= std::fmin(1.0f, std::fmax(0.0f, m.roughness_x)); // blend.cpp:54
	const bool d1	= mix_delta_only(mats, m.two_sided, depth + 1), d2 = mix_delta_only(mats, m.thin, depth + 1);
	const float a1 = add ? a : a * (1 - f), a2 = add ? a : a * f;
	const float b1 = add ? b * 0.5f : b * (1 - f), b2 = add ? b * 0.5f : b * f;
	if (d1 && d2) // form All: no leaf
		return;
	if (!d1 && !d2) { // form None: both, and no flag from below
		const bool first = add || f <= 0.5f;
		mix_flatten_into(mats, m.two_sided, a1, b1, symbol && first, false, row, depth + 1);
		mix_flatten_into(mats, m.thin, a2, b2, symbol && !first, false, row, depth + 1);
	} else if (d1) { // form First: child 2 alone
		mix_flatten_into(mats, m.thin, a2, b2, symbol, flag, row, depth + 1);
	} else { // form Second: child 1 alone
		mix_flatten_into(mats, m.two_sided, a1, b1, symbol, flag, row, depth + 1);
	}
}
inline MixRow mix_flatten(const prgpu_material* mats, uint32_t root)
{
	MixRow row;
	row.delta_only = mix_delta_only(mats, root);
	mix_flatten_into(mats, root, 1.0f, 1.0f, true, true, row);
	return row;
}
// A row as the device reads it (device/render.hip, vertex_eval): count, the root's delta-only bit, symbol leaf, flag leaf, then
// count x (leaf material, a, b).  Appends to `words`.
constexpr uint32_t MIX_ROW_HEADER = 4, MIX_ROW_LEAF = 3;
inline void mix_row_emit(const MixRow& row, std::vector<uint32_t>& words)
{
	auto bits = [](float v) {
		uint32_t u;
		static_assert(sizeof(u) == sizeof(v), "fp32");
		std::memcpy(&u, &v, sizeof(u));
		return u;
	};
	words.push_back((uint32_t)row.leaves.size());
	words.push_back(row.delta_only ? 1u : 0u);
	words.push_back(row.symbol_leaf);
	words.push_back(row.flag_leaf);
	for (const prgpu_mix_leaf& l : row.leaves) {
		words.push_back(l.material);
		words.push_back(bits(l.weight));
		words.push_back(bits(l.pdf));
	}
}
} // namespace prgpu_host
