// Calls every public method of groan::Msd (include/groan_hip.hpp) once: tests/test_msd_host.py compiles this with -Wall -Wextra -Werror
// (-fsyntax-only: the C++ mirror is header-only, what can break without a device is that it no longer compiles against groan_hip.h).
#include "groan_hip.hpp"

size_t msd_mirror(groan::System &system) {
    groan::Msd lateral(system, "Membrane", 128, GR_MSD_X | GR_MSD_Y | GR_MSD_NOJUMP);
    groan::Msd m(system, "Water", 64);
    std::vector<int> status;
    m.append(0, 32);
    m.append(32, 32, &status);
    m.set_launch(2, 3);
    const groan::Msd::Curve curve = m.msd(16), full = m.msd();
    const std::vector<double> origin = m.from_origin();
    const std::vector<float> d = m.displacements(0, 4);
    const uint64_t n = m.frames() + m.n_atoms() + m.capacity() + m.stat(GR_MSD_STAT_LAGS) + (m.raw_handle() ? 1u : 0u);
    m.clear();
    groan::Msd moved(std::move(m));
    return curve.msd.size() + curve.pairs.size() + full.msd.size() + origin.size() + d.size() + status.size() + (size_t)n + (size_t)moved.frames() + (size_t)lateral.capacity();
}
