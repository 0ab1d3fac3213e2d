// ukm_screen.h — the tile of ukm_screen.hip's reduction kernel.  tests/test_gpu_screen.py reads these lines and places its
// record boundaries on, beside and away from the tile edges: keep each constant on a line of its own.
#pragma once

constexpr int SCREEN_NT = 256;  // threads per workgroup
constexpr int SCREEN_VT = 8;    // consecutive windows per thread
constexpr int SCREEN_TILE = SCREEN_NT * SCREEN_VT;  // windows per workgroup
