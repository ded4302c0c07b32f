// vv_gate.h -- the numeric limits vv_render holds a frame to, by name: what vv_api.cpp tests on the host is what the device helpers' operand
// ranges are derived from (csrc/vv_device.h ph_div_core / ph_sqrt_core, chunk_count) and what host/device_math_check.hip sweeps.
#pragma once

namespace vv {

// every frame: a step below this (or not finite) is refused (vv_render)
constexpr float kStepMin = 1e-5f;
// FrameParams::safe_div (Phong): the gradient's divisions and square root run as their cores alone iff both pixel tangents lie in
// [kSafeDivTanLo, kSafeDivTanHi] and no step exceeds kSafeDivStepMax
constexpr float kSafeDivTanLo = 0x1p-24f;
constexpr float kSafeDivTanHi = 0x1p8f;
constexpr float kSafeDivStepMax = 16.f;

} // namespace vv
