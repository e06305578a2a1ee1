"""The postfix programs the host emits for trees of operator nodes (host/node_program.h through expr_emit of host/spectral_expr.h and scalar_emit
of host/scalar_node.h; DESIGN.md sections 2.8, 2.9), without a device: tests/node_program_check.cpp is compiled here with the host compiler and run.

Its printed text -- need, length and the words of a leaf, a unary over a leaf, the left- and the right-deep chain of five binary operators, the
balanced trees over eight and sixteen leaves, a unary over a binary over a unary, one node as both operands of its parent and 21 levels of
op(x, x), for both families -- equals tests/golden/node_programs.txt, which the same program printed when it was built against the headers of the
commit before the two families' emitters became one: the merged emitter is that commit's.  The program itself replays every program within the
device evaluators' bounds on a four-entry shift stack of its own and exits non-zero unless the result is the recursive evaluation's, bit for bit:
that is what the words mean."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_emitted_programs_are_the_recorded_ones_and_replay_to_the_recursion(tmp_path):
    exe = tmp_path / "node_program_check"
    # host code only (the shared arithmetic, device/node_math.h, needs the HIP headers for __host__ __device__); the library's floating-point flags
    subprocess.check_call([HIPCC, "--offload-host-only", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unused-function",
                           os.path.join(ROOT, "tests", "node_program_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "FAIL" not in r.stdout, r.stdout + r.stderr
    with open(os.path.join(ROOT, "tests", "golden", "node_programs.txt")) as f:
        assert r.stdout == f.read()
    # what the recorded text says, spelt out: chains need two entries, the left-deep one swaps nothing, the right-deep one every operator over
    # a subtree; eight leaves need 4 entries and 15 words, sixteen need 5 (refused by the callers), and the length saturates at 2^20
    tree = {m[0]: (m[1], m[2]) for m in re.findall(r"^(\S+ / [^:]+): (need \d+ length \d+)\n +([^\n]*)$", r.stdout, re.M)}
    assert len(tree) == 18
    for fam in ("spectral", "scalar"):
        assert tree[fam + " / left-deep chain of five"][0] == "need 2 length 11" and "~" not in tree[fam + " / left-deep chain of five"][1]
        right = tree[fam + " / right-deep chain of five"]
        assert right[0] == "need 2 length 11" and right[1].count("~") == 4   # (the innermost operator stands over two leaves: a tie, not swapped)
        assert tree[fam + " / balanced over eight leaves"][0] == "need 4 length 15"
        assert tree[fam + " / balanced over sixteen leaves"][0] == "need 5 length 31"
        assert tree[fam + " / one node as both operands"][0] == "need 3 length 7"
        assert tree[fam + " / 21 levels of op(x, x)"] == ("need 22 length %d" % (1 << 20), "not emitted")
