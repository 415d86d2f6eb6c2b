// Calls every public method of groan::VectorCorrelation (include/groan_hip.hpp) once: tests/test_vcorr_host.py compiles this with -Wall
// -Wextra -Werror (-fsyntax-only: the C++ mirror is header-only, what can break without a device is that it no longer compiles against
// groan_hip.h).
#include "groan_hip.hpp"

size_t vcorr_mirror(groan::System &system) {
    const std::vector<uint64_t> nh = { 0, 1, 7, 8, 15, 16 };
    groan::VectorCorrelation first(system, nh, 128, GR_VCORR_PBC | GR_VCORR_P1);
    groan::VectorCorrelation v(system, nh, 64);
    std::vector<int> status;
    v.append(0, 32);
    v.append(32, 32, &status);
    v.set_launch(2, 3, 4);
    const groan::VectorCorrelation::Curves curve = v.correlate(16), full = v.correlate();
    const groan::VectorCorrelation::Each each = v.correlate_each(8);
    const std::vector<float> u = v.vectors(0, 4);
    const uint64_t n = v.frames() + v.count() + v.capacity() + v.stat(GR_VCORR_STAT_LAGS) + (v.raw_handle() ? 1u : 0u);
    v.clear();
    groan::VectorCorrelation moved(std::move(v));
    return curve.c1.size() + curve.c2.size() + curve.pairs.size() + full.c1.size() + each.c1.size() + each.c2.size() + each.lags + u.size() + status.size() + (size_t)n +
           (size_t)moved.frames() + (size_t)first.capacity();
}
