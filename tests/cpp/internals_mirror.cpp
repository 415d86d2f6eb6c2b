// Calls every public method of groan::Internals (include/groan_hip.hpp) once: tests/test_internals_host.py compiles this with -Wall -Wextra
// -Werror (-fsyntax-only: the C++ mirror is header-only, what can break without a device is that it no longer compiles against groan_hip.h).
#include "groan_hip.hpp"

size_t internals_mirror(groan::System &system, float *out_dev) {
    const std::vector<uint64_t> phi = { 4, 6, 8, 14, 14, 16, 18, 24 }, bonds = { 0, 1, 1, 2 };
    const float normal[3] = { 0.0f, 0.0f, 1.0f };
    groan::Internals torsions(system, GR_IC_DIHEDRAL, phi);
    groan::Internals order(system, GR_IC_AXIS, bonds, GR_IC_PBC, normal), other(system, GR_IC_AXIS, bonds, GR_IC_PBC, normal);
    std::vector<int> status;
    const std::vector<float> series = torsions.values(0, 8), again = torsions.values(0, 8, &status);
    torsions.values_device(0, 8, out_dev, 64);
    torsions.values_device(0, 8, out_dev, 64, &status);
    torsions.set_launch(2, 3);
    order.accumulate(0, 4);
    other.accumulate(4, 4, &status);
    order.merge(other);
    const groan::Internals::Stats stats = order.read();
    const groan::Internals::Raw raw = order.raw();
    const std::vector<double> s = order.order_parameter();
    const uint64_t n = torsions.count() + order.frames() + torsions.stat(GR_IC_STAT_ARITY) + (torsions.raw_handle() ? 1u : 0u) + raw.n;
    other.clear();
    groan::Internals moved(std::move(other));
    return series.size() + again.size() + status.size() + stats.mean.size() + stats.var.size() + raw.origin.size() + raw.sum.size() + raw.sumsq.size() + s.size() + (size_t)n +
           (size_t)moved.count();
}
