// Calls every new gyration method of groan::Segments (include/groan_hip.hpp) once: tests/test_gyration_host.py compiles this with -Wall
// -Wextra -Werror (-fsyntax-only: the C++ mirror is header-only, what can break without a device is that it no longer compiles against
// groan_hip.h).
#include "groan_hip.hpp"

size_t gyration_mirror(groan::System &system) {
    groan::Segments seg = groan::Segments::from_lists(system, { { 0, 1, 2 }, { 5, 7 }, { 9 } });
    std::vector<int> status;
    seg.set_piece_frames(2);
    const groan::Segments::Gyration plain = seg.gyration(0, 4);
    const groan::Segments::Gyration full = seg.gyration(0, 4, groan::CenterKind::Estimate, false, true, &status);
    seg.set_piece_frames(0);
    const groan::Segments::GyrationDevice dev = seg.gyration_device(0, 4, groan::CenterKind::Naive, true, true, &status);
    const groan::Segments::GyrationDevice dev2 = seg.gyration_device(0, 1);
    return plain.moments.size() + plain.axes.size() + full.moments.size() + full.axes.size() + status.size() + (dev.moments ? 1u : 0u) + (dev.axes ? 1u : 0u) +
           (dev2.moments ? 1u : 0u) + (size_t)seg.stat(GR_SEG_STAT_LAST_PIECES);
}
