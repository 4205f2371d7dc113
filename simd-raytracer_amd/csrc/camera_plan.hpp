// The scalars a camera of `fov_degrees` makes rays from over a width x height raster, one copy for the calls that shoot the rays
// (api_frame.hip camera_args) and the one that undoes them (temporal_plan.hpp).  Plain host arithmetic, no HIP.
#pragma once

#include <cmath>
#include <cstdint>

namespace rtk {

struct CameraScalars { float aspect, tan_half_fov, width_f, height_f; };

inline CameraScalars camera_scalars(uint32_t width, uint32_t height, double fov_degrees) {
    CameraScalars c;
    c.aspect = static_cast<float>(width) / static_cast<float>(height);                       // render.hpp:26
    // render.hpp:55-57: `const F fov_radians = degrees_to_radians(fov_degrees)` is evaluated in double (fov_degrees is a
    // double constant, utils/convert.hpp:4-6) and ROUNDED TO FLOAT by the declaration; `std::tan(fov_radians / F(2))` is
    // then the float overload (tanf), and `screen_x *=` a float multiply (common.hip.hpp camera_ray).
    const float fov_radians = static_cast<float>(fov_degrees * (3.14159265358979323846 / 180.0));
    c.tan_half_fov = std::tan(fov_radians / 2.0f);
    c.width_f = static_cast<float>(width); c.height_f = static_cast<float>(height);
    return c;
}

}  // namespace rtk
