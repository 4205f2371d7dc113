// The nine build-time constants of the reference's raytracer/config.hpp, settable with -D.  This directory precedes the
// reference's include directory on the probe's include path, so its headers pick this file up; the defaults are its values.
#pragma once

#include <cstddef>
#include <optional>

#ifndef RTK_REF_FOV_DEGREES
#define RTK_REF_FOV_DEGREES 90.
#endif
#ifndef RTK_REF_EPSILON
#define RTK_REF_EPSILON 1e-6
#endif
#ifndef RTK_REF_SHADOW_BIAS
#define RTK_REF_SHADOW_BIAS 1e-4
#endif
#ifndef RTK_REF_REFLECTION_BIAS
#define RTK_REF_REFLECTION_BIAS 1e-4
#endif
#ifndef RTK_REF_REFRACTION_BIAS
#define RTK_REF_REFRACTION_BIAS 1e-4
#endif
#ifndef RTK_REF_SAMPLES_PER_PIXEL
#define RTK_REF_SAMPLES_PER_PIXEL 1
#endif
#ifndef RTK_REF_MAX_RAY_DEPTH
#define RTK_REF_MAX_RAY_DEPTH 5
#endif
#ifndef RTK_REF_DIFFUSE_RAY_COUNT
#define RTK_REF_DIFFUSE_RAY_COUNT 0
#endif
#ifndef RTK_REF_RNG_SEED
#define RTK_REF_RNG_SEED 42
#endif

constexpr double fov_degrees = RTK_REF_FOV_DEGREES;

constexpr double epsilon = RTK_REF_EPSILON;
constexpr double shadow_bias = RTK_REF_SHADOW_BIAS;
constexpr double reflection_bias = RTK_REF_REFLECTION_BIAS;
constexpr double refraction_bias = RTK_REF_REFRACTION_BIAS;

constexpr std::size_t samples_per_pixel = RTK_REF_SAMPLES_PER_PIXEL;
constexpr std::size_t max_ray_depth = RTK_REF_MAX_RAY_DEPTH;
constexpr std::size_t diffuse_reflection_ray_count = RTK_REF_DIFFUSE_RAY_COUNT;

constexpr std::optional fixed_rng_seed = std::make_optional(RTK_REF_RNG_SEED);
