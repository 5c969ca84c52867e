// Camera set-up and staging layouts of the host API (semtsdf_api.cpp) on plain arrays.  Host code
// only, no HIP: tests/helpers/api_parts_check.cpp compiles it alone.
#pragma once

#include <cstddef>
#include <cstdint>

namespace semtsdf {

// The 3x3 part of a row-major 4x4 (K, K^-1).
inline void cam_mat3(float dst[9], const float m[16]) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) dst[i * 3 + j] = m[i * 4 + j];
}

// A view's camera (MarchCamera): rows 0..2 of screen-to-world, the centre as the ray origin.
template <class Cam>
void cam_view(Cam& m, const float s2w[16], const float c[3]) {
    for (int i = 0; i < 12; ++i) m.s2w[i] = s2w[i];
    for (int i = 0; i < 3; ++i) m.o[i] = c[i];
    m.use_s2w = 1;
}

// The inverse of a pose E = [R | t]: Rt = R^T and o = -Rt t, each o[i] a left-to-right sum of three
// double products rounded once (cv::gemm on CV_32F, tsdf.cu:432-435).  Two forms of o, equal but for
// the sign of a zero when all three products are -0.0:
//   cam_origin        (float)(-(0.0 + p0 + p1 + p2))  semtsdf_pose_camera, the ICP system: -0.0f there
//   cam_origin_assoc  -(float)(p0 + p1 + p2)          the association march:               +0.0f there
inline void cam_rt(float Rt[9], const float E[16]) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Rt[i * 3 + j] = E[j * 4 + i];
}
inline void cam_origin(float o[3], const float E[16]) {
    for (int i = 0; i < 3; ++i) {
        double acc = 0;
        for (int k = 0; k < 3; ++k) acc += (double)E[k * 4 + i] * (double)E[k * 4 + 3];
        o[i] = (float)(-acc);
    }
}
inline void cam_origin_assoc(float o[3], const float E[16]) {
    for (int i = 0; i < 3; ++i)
        o[i] = -(float)((double)E[i] * (double)E[3] + (double)E[4 + i] * (double)E[7] + (double)E[8 + i] * (double)E[11]);
}

// Bump carver of one staging allocation for n pixels: typed sub-arrays of per_px * n + fixed
// elements in the order asked for, each at its natural alignment, and the bytes used so far.  A null
// base only measures.  The layouts below carve in declaration order; their bytes is the total.
struct Carver {
    Carver(void* base, size_t n) : base(static_cast<char*>(base)), n(n) {}
    char* base;
    size_t n, bytes = 0;
    template <class T>
    T* take(size_t per_px, size_t fixed = 0) {
        bytes = (bytes + alignof(T) - 1) / alignof(T) * alignof(T);
        T* p = base ? reinterpret_cast<T*>(base + bytes) : nullptr;
        bytes += (per_px * n + fixed) * sizeof(T);
        return p;
    }
};

// semtsdf_render_maps: the six maps, 34 B per pixel.
struct MapsScratch {
    Carver c;
    float *t = c.take<float>(1), *point = c.take<float>(3), *normal = c.take<float>(3), *votes = c.take<float>(1);
    uint8_t *label = c.take<uint8_t>(1), *flags = c.take<uint8_t>(1);
    size_t bytes = c.bytes;
};

// semtsdf_frame_maps and semtsdf_icp_system: frame and model maps, the system's words, the two flag
// maps and the depth image, 52 B per pixel + 8 B per word.
struct TrackScratch {
    Carver c;
    size_t nwords;
    float *vertex = c.take<float>(3), *normal = c.take<float>(3), *m_point = c.take<float>(3), *m_normal = c.take<float>(3);
    int64_t* words = c.take<int64_t>(0, nwords);
    uint8_t *flags = c.take<uint8_t>(1), *m_flags = c.take<uint8_t>(1);
    uint16_t* depth = c.take<uint16_t>(1);
    size_t bytes = c.bytes;
};

// The inverse camera matrix of pyramid level l >= 1 (row-major 3x3) from the 4x4 K of level 0: the
// focal lengths halve per level and a coarse pixel covers the fine pixels 2x and 2x + 1 (pixel centres
// at integers), so c_l = (c + 0.5) / 2^l - 0.5.  Formed in double, each entry rounded once.
inline void cam_level_kinv(float dst[9], const float K[16], int level) {
    const double s = (double)(1 << level);
    const double fx = (double)K[0] / s, fy = (double)K[5] / s;
    const double cx = ((double)K[2] + 0.5) / s - 0.5, cy = ((double)K[6] + 0.5) / s - 0.5;
    const double m[9] = {1.0 / fx, 0.0, -cx / fx, 0.0, 1.0 / fy, -cy / fy, 0.0, 0.0, 1.0};
    for (int i = 0; i < 9; ++i) dst[i] = (float)m[i];
}

// semtsdf_frame_pyramid: z and the three maps of every level the image admits (29 B per pixel of a
// level, at most kLevels of them) and the depth image.
struct PyramidScratch {
    static constexpr int kLevels = 4;  // SEMTSDF_PYRAMID_MAX_LEVELS
    Carver c;
    float *z[kLevels], *vertex[kLevels], *normal[kLevels];
    uint8_t* flags[kLevels];
    uint16_t* depth;
    size_t bytes;
    PyramidScratch(void* base, int width, int height) : c(base, 0) {
        size_t n[kLevels];
        for (int l = 0; l < kLevels; ++l) n[l] = (size_t)(width >> l) * (size_t)(height >> l);
        for (int l = 0; l < kLevels; ++l) z[l] = c.take<float>(0, n[l]);
        for (int l = 0; l < kLevels; ++l) vertex[l] = c.take<float>(0, 3 * n[l]);
        for (int l = 0; l < kLevels; ++l) normal[l] = c.take<float>(0, 3 * n[l]);
        depth = c.take<uint16_t>(0, n[0]);
        for (int l = 0; l < kLevels; ++l) flags[l] = c.take<uint8_t>(0, n[l]);
        bytes = c.bytes;
    }
};

// The camera of pyramid level l >= 0 (fx, fy, cx, cy) by cam_level_kinv's rule, each rounded once.
inline void cam_level(float out[4], const float K[16], int level) {
    const double s = (double)(1 << level);
    out[0] = (float)((double)K[0] / s);
    out[1] = (float)((double)K[5] / s);
    out[2] = (float)(((double)K[2] + 0.5) / s - 0.5);
    out[3] = (float)(((double)K[6] + 0.5) / s - 0.5);
}

// semtsdf_intensity_pyramid and semtsdf_rgbd_system_level: the colour image and its validity (4 B per
// pixel), S and valid of every level the image admits (5 B per pixel of a level), and the system's
// four intensity arrays of one level (10 B per pixel) with its words.
struct IntensityScratch {
    static constexpr int kLevels = 4;  // SEMTSDF_PYRAMID_MAX_LEVELS
    Carver c;
    int64_t* words;
    uint32_t *S[kLevels], *f_S, *m_S;
    uint8_t *ok[kLevels], *f_ok, *m_ok, *rgb, *valid;
    size_t bytes;
    IntensityScratch(void* base, int width, int height, size_t nwords) : c(base, 0) {
        size_t n[kLevels];
        for (int l = 0; l < kLevels; ++l) n[l] = (size_t)(width >> l) * (size_t)(height >> l);
        words = c.take<int64_t>(0, nwords);
        for (int l = 0; l < kLevels; ++l) S[l] = c.take<uint32_t>(0, n[l]);
        f_S = c.take<uint32_t>(0, n[0]);
        m_S = c.take<uint32_t>(0, n[0]);
        for (int l = 0; l < kLevels; ++l) ok[l] = c.take<uint8_t>(0, n[l]);
        f_ok = c.take<uint8_t>(0, n[0]);
        m_ok = c.take<uint8_t>(0, n[0]);
        rgb = c.take<uint8_t>(0, 3 * n[0]);
        valid = c.take<uint8_t>(0, n[0]);
        bytes = c.bytes;
    }
};

// The sharded ray protocol's per-pixel march state (ShardRayState), 24 B per pixel.
struct RayScratch {
    Carver c;
    int* k = c.take<int>(1);
    float* fk = c.take<float>(1);
    int* j = c.take<int>(1);
    float *fj = c.take<float>(1), *fp = c.take<float>(1), *t = c.take<float>(1);
    size_t bytes = c.bytes;
};

}  // namespace semtsdf

