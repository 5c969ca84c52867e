// Stand-alone check of the host API's camera helpers and staging layouts (csrc/semtsdf_cam.h).
// Cameras: each helper against the expression its call sites in semtsdf_api.cpp held before the
// helpers existed, written out below, bit for bit (memcmp, so the sign of a zero counts), for five
// inputs.  Layouts: every offset against the documented table, alignment, no overlap and the total, at
// three pixel counts.  A sanitizer build sees any read or write outside the arrays.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../slam-maskrcnn_amd/csrc/semtsdf_cam.h"

using namespace semtsdf;

static int g_failures = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            ++g_failures;                                            \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);    \
        }                                                            \
    } while (0)

struct Cam {  // the fields of MarchCamera
    float Kinv[9], Rt[9], o[3], s2w[12];
    int use_s2w;
};

// ---- the former call-site expressions
static void ref_mat3_listed(float d[9], const float* K) {  // integrate_impl, assoc_camera
    d[0] = K[0]; d[1] = K[1]; d[2] = K[2];
    d[3] = K[4]; d[4] = K[5]; d[5] = K[6];
    d[6] = K[8]; d[7] = K[9]; d[8] = K[10];
}
static void ref_mat3_loop(float d[9], const float* K) {  // frame_maps_impl, icp_impl
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) d[i * 3 + j] = K[i * 4 + j];
}
static void ref_view(Cam& m, const float* s2w, const float* c) {  // render_args, maps_impl, shard_ray_begin
    for (int i = 0; i < 12; ++i) m.s2w[i] = s2w[i];
    m.o[0] = c[0]; m.o[1] = c[1]; m.o[2] = c[2];
    m.use_s2w = 1;
}
static void ref_assoc(float Rt[9], float o[3], const float* E) {  // assoc_camera
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Rt[i * 3 + j] = E[j * 4 + i];
    for (int i = 0; i < 3; ++i) {
        const double acc = (double)Rt[i * 3 + 0] * (double)E[3] + (double)Rt[i * 3 + 1] * (double)E[7] +
                           (double)Rt[i * 3 + 2] * (double)E[11];
        o[i] = -(float)acc;
    }
}
static void ref_pose(float o[3], const float* E) {  // semtsdf_pose_camera
    for (int i = 0; i < 3; ++i) {
        double acc = 0;
        for (int k = 0; k < 3; ++k) acc += (double)E[k * 4 + i] * (double)E[k * 4 + 3];
        o[i] = (float)(-acc);
    }
}
static void ref_icp(float Rt[9], float o[3], const float* E) {  // icp_impl
    for (int i = 0; i < 3; ++i) {
        double acc = 0;
        for (int k = 0; k < 3; ++k) acc += (double)E[k * 4 + i] * (double)E[k * 4 + 3];
        o[i] = (float)(-acc);
        for (int j = 0; j < 3; ++j) Rt[i * 3 + j] = E[j * 4 + i];
    }
}

static bool same(const void* a, const void* b, size_t n) { return memcmp(a, b, n) == 0; }

static void check_pose(const char* name, const float E[16], const float K[16]) {
    const int before = g_failures;
    float a[9], b[9], c[9], oa[3], ob[3];
    cam_mat3(a, K);
    ref_mat3_listed(b, K);
    ref_mat3_loop(c, K);
    CHECK(same(a, b, sizeof(a)) && same(a, c, sizeof(a)));
    cam_rt(a, E);
    cam_origin_assoc(oa, E);
    ref_assoc(b, ob, E);
    CHECK(same(a, b, sizeof(a)) && same(oa, ob, sizeof(oa)));
    cam_origin(oa, E);
    ref_pose(ob, E);
    CHECK(same(oa, ob, sizeof(oa)));
    ref_icp(b, ob, E);
    CHECK(same(a, b, sizeof(a)) && same(oa, ob, sizeof(oa)));
    Cam m, r;  // the view: E's rows as a screen-to-world matrix, K's first row as the centre
    memset(&m, 0, sizeof(m));
    memset(&r, 0, sizeof(r));
    cam_view(m, E, K);
    ref_view(r, E, K);
    CHECK(same(&m, &r, sizeof(m)));
    printf("camera %s %s\n", name, g_failures == before ? "ok" : "FAILED");
}

// ---- layouts
struct Part {
    const char* name;
    const void* p;
    size_t elem, count, want;  // element size, elements, documented offset
};

static void check_layout(const char* name, size_t n, const char* base, size_t bytes, size_t want_bytes,
                         std::vector<Part> parts) {
    const int before = g_failures;
    CHECK(bytes == want_bytes);
    for (const Part& q : parts) {
        const size_t off = (size_t)((const char*)q.p - base);
        if (off != q.want) printf("%s %s at %zu, documented at %zu\n", name, q.name, off, q.want);
        CHECK(off == q.want);
        CHECK(off % q.elem == 0);
        CHECK(off + q.elem * q.count <= bytes);
    }
    std::sort(parts.begin(), parts.end(), [](const Part& a, const Part& b) { return a.p < b.p; });
    for (size_t i = 0; i + 1 < parts.size(); ++i)
        CHECK((const char*)parts[i].p + parts[i].elem * parts[i].count <= (const char*)parts[i + 1].p);
    printf("layout %s n=%zu %s\n", name, n, g_failures == before ? "ok" : "FAILED");
}

static void check_layouts(size_t n) {
    const size_t W = 32;  // kIcpWords
    std::vector<char> buf(52 * n + 8 * W);
    char* base = buf.data();
    memset(base, 0, buf.size());
    CHECK((uintptr_t)base % 8 == 0);
    {
        CHECK((MapsScratch{{nullptr, n}}.bytes == 34 * n));
        const MapsScratch m{{base, n}};
        check_layout("maps", n, base, m.bytes, 34 * n,
                     {{"t", m.t, 4, n, 0}, {"point", m.point, 4, 3 * n, 4 * n}, {"normal", m.normal, 4, 3 * n, 16 * n},
                      {"votes", m.votes, 4, n, 28 * n}, {"label", m.label, 1, n, 32 * n}, {"flags", m.flags, 1, n, 33 * n}});
        m.t[n - 1] = 1.0f; m.votes[n - 1] = 1.0f; m.flags[n - 1] = 1;  // the ends, under the sanitizer
    }
    {
        CHECK((TrackScratch{{nullptr, n}, W}.bytes == 52 * n + 8 * W));
        const TrackScratch t{{base, n}, W};
        check_layout("tracking", n, base, t.bytes, 52 * n + 8 * W,
                     {{"vertex", t.vertex, 4, 3 * n, 0}, {"normal", t.normal, 4, 3 * n, 12 * n},
                      {"m_point", t.m_point, 4, 3 * n, 24 * n}, {"m_normal", t.m_normal, 4, 3 * n, 36 * n},
                      {"words", t.words, 8, W, 48 * n}, {"flags", t.flags, 1, n, 48 * n + 8 * W},
                      {"m_flags", t.m_flags, 1, n, 49 * n + 8 * W}, {"depth", t.depth, 2, n, 50 * n + 8 * W}});
        t.words[W - 1] = 1; t.m_flags[n - 1] = 1; t.depth[n - 1] = 1;
    }
    {
        CHECK((RayScratch{{nullptr, n}}.bytes == 24 * n));
        const RayScratch r{{base, n}};
        check_layout("ray", n, base, r.bytes, 24 * n,
                     {{"k", r.k, 4, n, 0}, {"fk", r.fk, 4, n, 4 * n}, {"j", r.j, 4, n, 8 * n}, {"fj", r.fj, 4, n, 12 * n},
                      {"fp", r.fp, 4, n, 16 * n}, {"t", r.t, 4, n, 20 * n}});
        r.t[n - 1] = 1.0f;
    }
}

int main() {
    const float pinhole[16] = {520.9f, 0, 325.1f, 0, 0, 521.0f, 249.7f, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    const float skewed[16] = {520.9f, 0.37f, 325.1f, 0.5f, -0.011f, 521.0f, 249.7f, -2.0f,
                              1e-4f, -2e-4f, 0.99f, 3.0f, 7.0f, 8.0f, 9.0f, 1.0f};  // no pinhole: every entry set
    const float identity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    const float general[16] = {0.9362934f, -0.2896295f, 0.1986693f, 0.1234567f, 0.3129918f, 0.9447025f, -0.0978434f,
                               -2.7182818f, -0.1593451f, 0.1537920f, 0.9751703f, 3.1415927f, 0, 0, 0, 1};
    // t = +0 and a rotation column (column 1) without a positive entry: all three products are -0.0
    const float negcol[16] = {1, -0.6f, 0, 0.0f, 0, -0.8f, 1, 0.0f, 0, -0.0f, 0, 0.0f, 0, 0, 0, 1};
    const float negzero_t[16] = {0.9362934f, -0.2896295f, 0.1986693f, -0.0f, 0.3129918f, 0.9447025f, -0.0978434f, -0.0f,
                                 -0.1593451f, 0.1537920f, 0.9751703f, -0.0f, 0, 0, 0, 1};
    check_pose("identity", identity, pinhole);
    check_pose("general", general, pinhole);
    check_pose("negative-column", negcol, pinhole);
    check_pose("negative-zero-t", negzero_t, pinhole);
    check_pose("non-pinhole-K", general, skewed);
    {  // where the two forms of the origin part: -0.0f (pose, ICP) against +0.0f (association)
        float op[3], oa[3];
        cam_origin(op, negcol);
        cam_origin_assoc(oa, negcol);
        uint32_t bp, ba;
        memcpy(&bp, &op[1], 4);
        memcpy(&ba, &oa[1], 4);
        CHECK(bp == 0x80000000u && ba == 0u);
        printf("origin forms at the all-negative column: pose %08x assoc %08x\n", bp, ba);
    }
    for (size_t n : {(size_t)1, (size_t)75 * 53, (size_t)640 * 480}) check_layouts(n);
    printf("failures %d\n", g_failures);
    return g_failures ? 1 : 0;
}
