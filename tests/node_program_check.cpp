// node_program_check.cpp -- what the host emits for a tree of operator nodes, for BOTH node families (spectral expressions: spectral_expr.h;
// scalar nodes: scalar_node.h), and what those words mean.  A stand-alone host program (tests/test_node_program.py compiles and runs it):
// for every tree below it prints need, length and the program's words -- the text tests/golden/node_programs.txt pins -- and, for a tree
// within the device evaluators' bounds, replays the program on a four-entry shift stack WRITTEN HERE (a restatement of expr_eval /
// scalar_run of device/render.hip, on purpose) with the shared expr_op / scalar_op, and exits non-zero unless the result equals the
// recursive evaluation bit for bit at 400, 550 and 700 nm.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../include/prgpu.h"
#include "../pearray_amd/csrc/host/scalar_node.h"
#include "../pearray_amd/csrc/host/spectral_expr.h"

namespace prd {
}
using namespace prgpu_host;
using namespace prd;

namespace {
std::vector<prgpu_spectrum> nodes;
uint32_t add(uint32_t kind, uint32_t lhs = PRGPU_INVALID_ID, uint32_t rhs = PRGPU_INVALID_ID, float p0 = 0.0f)
{
	prgpu_spectrum s;
	std::memset(&s, 0, sizeof(s));
	s.kind = kind;
	s.lhs  = lhs;
	s.rhs  = rhs;
	s.p[0] = p0;
	nodes.push_back(s);
	return uint32_t(nodes.size() - 1);
}
// distinct constant leaves: 1.25, 1.75, 2.25, ... by position in the array (report() refuses a tree that evaluates to no number)
uint32_t leaf() { return add(PRGPU_SPEC_CONST, PRGPU_INVALID_ID, PRGPU_INVALID_ID, 1.25f + 0.5f * float(nodes.size() % 61)); }

// One family: its operators for the trees (three non-commutative binary ones, cycled; one unary), its sizing, emission and the two evaluations.
struct Family {
	const char* name;
	uint32_t binary[3], unary;
	bool scalar;
};
const Family SPECTRAL = { "spectral", { PRGPU_SPEC_SUB, PRGPU_SPEC_DIV, PRGPU_SPEC_SUB }, PRGPU_SPEC_NEG, false };
const Family SCALAR	  = { "scalar", { PRGPU_SPEC_SCALAR_SUB, PRGPU_SPEC_SCALAR_DIV, PRGPU_SPEC_SCALAR_POW }, PRGPU_SPEC_SCALAR_NEG, true };

uint32_t bin(const Family& f, uint32_t a, uint32_t b) { return add(f.binary[nodes.size() % 3], a, b); }
uint32_t balanced(const Family& f, int leaves) // (the left subtree's nodes first: no two calls in one argument list)
{
	if (leaves == 1)
		return leaf();
	const uint32_t a = balanced(f, leaves / 2);
	const uint32_t b = balanced(f, leaves / 2);
	return bin(f, a, b);
}

struct Extent {
	uint32_t need, length;
};
float scalar_eval_at(uint32_t id) // the scalar recursion: FloatScalarNode::eval over constants
{
	const prgpu_spectrum& n = nodes[id];
	if (!scalar_is_op(n.kind))
		return n.p[0];
	return scalar_op(n.kind, scalar_eval_at(n.lhs), scalar_is_unary(n.kind) ? 0.0f : scalar_eval_at(n.rhs));
}
// the device's stack machine, restated: four entries that shift, s[0] the top
float replay(const Family& f, const std::vector<uint32_t>& words)
{
	float s[4] = { 0, 0, 0, 0 };
	for (uint32_t word : words) {
		const prgpu_spectrum& n = nodes[word & 0x00FFFFFFu];
		const bool op			= f.scalar ? scalar_is_op(n.kind) : spec_is_math(n.kind);
		if (!op) {
			s[3] = s[2], s[2] = s[1], s[1] = s[0], s[0] = n.p[0];
			continue;
		}
		const bool unary = f.scalar ? scalar_is_unary(n.kind) : spec_is_unary(n.kind);
		const bool swap	 = (word & 0x80000000u) != 0u;
		const float a = unary ? s[0] : (swap ? s[0] : s[1]), b = swap ? s[1] : s[0];
		s[0] = f.scalar ? scalar_op(n.kind, a, b) : expr_op(n.kind, a, b, n.p[0], n.p[1]);
		if (!unary)
			s[1] = s[2], s[2] = s[3];
	}
	return s[0];
}

int failures = 0;
void report(const Family& f, const char* tree, uint32_t root)
{
	std::vector<ExprInfo> einfo;
	std::vector<ScalarInfo> sinfo;
	for (const prgpu_spectrum& n : nodes) {
		einfo.push_back(expr_info_of(n, einfo, nodes.data()));
		sinfo.push_back(scalar_info_of(n, sinfo));
	}
	const Extent x = f.scalar ? Extent{ sinfo[root].need, sinfo[root].length } : Extent{ einfo[root].need, einfo[root].length };
	std::printf("%s / %s: need %u length %u\n", f.name, tree, x.need, x.length);
	if (x.length > 256u) { // (2^20 words and more: sized, never emitted -- the callers refuse it on its length)
		std::printf("  not emitted\n");
		return;
	}
	std::vector<uint32_t> words;
	if (f.scalar)
		scalar_emit(nodes.data(), sinfo, root, words);
	else
		expr_emit(nodes.data(), einfo, root, words);
	std::printf(" ");
	for (uint32_t w : words)
		std::printf(" %s%u:%u", (w & 0x80000000u) ? "~" : "", w & 0x00FFFFFFu, nodes[w & 0x00FFFFFFu].kind);
	std::printf("\n");
	if (words.size() != x.length) {
		std::printf("  FAIL: %zu words emitted\n", words.size());
		++failures;
	}
	if (x.need > PRGPU_EXPR_MAX_STACK || x.length > PRGPU_EXPR_MAX_PROGRAM)
		return;
	for (float wl : { 400.0f, 550.0f, 700.0f }) {
		const float want = f.scalar ? scalar_eval_at(root) : expr_eval_at(nodes.data(), uint32_t(nodes.size()), root, wl, [](const prgpu_spectrum& l, float) { return l.p[0]; });
		const float got	 = replay(f, words);
		if (want != want) {
			std::printf("  FAIL at %g nm: the tree evaluates to no number and checks nothing\n", wl);
			++failures;
		}
		if (std::memcmp(&want, &got, 4) != 0) {
			std::printf("  FAIL at %g nm: the program gives %.9g, the recursion %.9g\n", wl, got, want);
			++failures;
		}
	}
}

void family(const Family& f)
{
	nodes.clear();
	report(f, "a leaf", leaf());
	report(f, "a unary over a leaf", add(f.unary, leaf()));
	uint32_t chain = leaf();
	for (int k = 0; k < 5; ++k)
		chain = bin(f, chain, leaf());
	report(f, "left-deep chain of five", chain);
	chain = leaf();
	for (int k = 0; k < 5; ++k)
		chain = bin(f, leaf(), chain);
	report(f, "right-deep chain of five", chain);
	report(f, "balanced over eight leaves", balanced(f, 8));
	const uint32_t inner = add(f.unary, leaf());
	report(f, "unary over binary over unary", add(f.unary, bin(f, inner, leaf())));
	const uint32_t shared = balanced(f, 2);
	report(f, "one node as both operands", bin(f, shared, shared));
	report(f, "balanced over sixteen leaves", balanced(f, 16));
	uint32_t x = leaf();
	for (int k = 0; k < 21; ++k)
		x = bin(f, x, x);
	report(f, "21 levels of op(x, x)", x);
}
} // namespace

int main()
{
	family(SPECTRAL);
	family(SCALAR);
	return failures ? 1 : 0;
}
