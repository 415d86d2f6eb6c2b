"""The C++ mirror of the hydrogen-bond plan (include/groan_hip.hpp: groan::HBondPlan) compiles against the C ABI as a user
would write it: a plan over chains of group names, pairs and the system's bonds, one batch call, the HBondMap per frame."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SNIPPET = r"""
#include "groan_hip.hpp"
#include <cstdio>
int main() {
    groan::System system(9);
    std::vector<groan::HBondChain> chains = {{"OW", "OW", "HW"}, {"N", "N", "H"}};
    std::vector<std::pair<uint32_t, uint32_t>> pairs = {{0, 0}, {0, 1}};
    std::vector<std::pair<uint64_t, uint64_t>> bonds = {{0, 1}, {0, 2}, {3, 4}};
    groan::HBondPlan plan(system, chains, pairs, bonds, 0.3f, 150.0f);
    std::vector<int> status;
    auto frames = plan.batch(0, 4, &status);
    for (size_t f = 0; f < frames.size(); ++f)
        for (size_t p = 0; p < plan.pairs().size(); ++p)
            for (const groan::HBond &b : frames[f][p]) std::printf("%u %u %u %f %f %d\n", b.donor, b.hydrogen, b.acceptor, b.distance, b.angle, status[f]);
    try { groan::HBondPlan bad(system, chains, {{0, 0}}, bonds, 0.3f, 150.0f); } catch (const groan::Error &e) { return e.variant == "UnusedChain" ? 0 : 1; }
    groan::HBondPlan moved = std::move(plan);
    return moved.raw() == nullptr;
}
"""


def test_hbond_plan_snippet_compiles(tmp_path):
    src = tmp_path / "hbond_snippet.cpp"
    src.write_text(SNIPPET)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
