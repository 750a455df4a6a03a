// fp32 geometry shared by the triangulation (nrs_triang.hip) and the map initialisation (nrs_init.hip): Sophus SE3f algebra, the
// cameras' Unproject, TriangulateMidPoint and RaysParallax.  Contraction off: the operation order of oracle/triang_oracle.py.
#pragma once
#include <cmath>
#include "nrs_device.hpp"

namespace nrs {

// ---- Sophus SE3f in float (so3.hpp:388-395, se3.hpp:222-225), contraction off
struct Se3f { float q[4], t[3]; };
__device__ inline void crossf(const float* a, const float* b, float* o) {
#pragma clang fp contract(off)
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ inline void so3_point(const float* q, const float* p, float* o) {
#pragma clang fp contract(off)
    float uv[3], c[3];
    crossf(q, p, uv);
    uv[0] = uv[0] + uv[0]; uv[1] = uv[1] + uv[1]; uv[2] = uv[2] + uv[2];
    crossf(q, uv, c);
    o[0] = p[0] + q[3] * uv[0] + c[0]; o[1] = p[1] + q[3] * uv[1] + c[1]; o[2] = p[2] + q[3] * uv[2] + c[2];
}
__device__ inline void se3_point(const Se3f& T, const float* p, float* o) {
#pragma clang fp contract(off)
    so3_point(T.q, p, o);
    o[0] = o[0] + T.t[0]; o[1] = o[1] + T.t[1]; o[2] = o[2] + T.t[2];
}
__device__ inline Se3f se3_inv(const Se3f& T) {
#pragma clang fp contract(off)
    Se3f r;
    r.q[0] = -T.q[0]; r.q[1] = -T.q[1]; r.q[2] = -T.q[2]; r.q[3] = T.q[3];
    const float nt[3] = {T.t[0] * -1.f, T.t[1] * -1.f, T.t[2] * -1.f};
    so3_point(r.q, nt, r.t);
    return r;
}
__device__ inline Se3f se3_mul(const Se3f& A, const Se3f& B) {
#pragma clang fp contract(off)
    Se3f r;
    const float* a = A.q; const float* b = B.q;
    r.q[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    r.q[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    r.q[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
    r.q[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
    float rt[3];
    so3_point(A.q, B.t, rt);
    r.t[0] = rt[0] + A.t[0]; r.t[1] = rt[1] + A.t[1]; r.t[2] = rt[2] + A.t[2];
    return r;
}
__device__ inline float normf3(const float* v) {
#pragma clang fp contract(off)
    return sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
}

// CameraModel::Unproject (pin_hole.cc:33-38, kannala_brandt_8.cc:53-85)
__device__ inline void unproject_f32(const Cam& c, float u, float v, float* ray) {
#pragma clang fp contract(off)
    const float x = (u - c.p[2]) / c.p[0], y = (v - c.p[3]) / c.p[1];
    if (c.model == 0) { ray[0] = x; ray[1] = y; ray[2] = 1.f; return; }
    const float theta_d = sqrtf(x * x + y * y);
    float th = 0.f;
    if (theta_d > 1e-8f) {
        float theta = theta_d;
        for (int j = 0; j < 10; ++j) {
            const float t2 = theta * theta, t4 = t2 * t2, t6 = t4 * t2, t8 = t4 * t4;
            const float a = c.p[4] * t2, b = c.p[5] * t4, cc = c.p[6] * t6, d = c.p[7] * t8;
            const float fix = (theta * (1.f + a + b + cc + d) - theta_d) / (1.f + 3.f * a + 5.f * b + 7.f * cc + 9.f * d);
            theta = theta - fix;
            if (fabsf(fix) < 1e-6f) break;
        }
        th = theta;
    }
    const float s = (float)sin((double)th), co = (float)cos((double)th);
    ray[0] = s * x / theta_d; ray[1] = s * y / theta_d; ray[2] = co;
}

// TriangulateMidPoint(ray_1, ray_2, camera1_transform_world, camera2_transform_world)  (geometry_toolbox.cc:45-79)
__device__ inline void triangulate_mid_point_f32(const float* ray_1, const float* ray_2, const Se3f& T1, const Se3f& T2, float* X) {
#pragma clang fp contract(off)
    float f0[3] = {ray_1[0], ray_1[1], ray_1[2]}, f1[3] = {ray_2[0], ray_2[1], ray_2[2]};
    float nn = normf3(f0); f0[0] /= nn; f0[1] /= nn; f0[2] /= nn;
    nn = normf3(f1); f1[0] /= nn; f1[1] /= nn; f1[2] /= nn;
    const Se3f T10 = se3_mul(T2, se3_inv(T1));
    const float x = T10.q[0], y = T10.q[1], z = T10.q[2], w = T10.q[3];
    const float tx = 2.f * x, ty = 2.f * y, tz = 2.f * z, twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x,
                tyy = ty * y, tyz = tz * y, tzz = tz * z;
    const float R[9] = {1.f - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.f - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1.f - (txx + tyy)};
    float Rf0[3];
    for (int i = 0; i < 3; ++i) Rf0[i] = (R[3 * i] * f0[0] + R[3 * i + 1] * f0[1]) + R[3 * i + 2] * f0[2];
    float p[3], q[3], r[3];
    crossf(Rf0, f1, p); crossf(Rf0, T10.t, q); crossf(f1, T10.t, r);
    const float nq = normf3(q), nr = normf3(r), np_ = normf3(p);
    const float s1 = nq / (nq + nr), s2 = nr / np_;
    float x1[3];
    for (int i = 0; i < 3; ++i) x1[i] = s1 * (T10.t[i] + s2 * (Rf0[i] + f1[i]));
    se3_point(se3_inv(T2), x1, X);
}

// RaysParallax (geometry_toolbox.cc:37-43): std::min(cs, 1.f) keeps a NaN cosine, which then passes every `<` gate, as in the reference
__device__ inline float rays_parallax_f32(const float* a, const float* b) {
#pragma clang fp contract(off)
    const float dot = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
    const float cs = dot / (normf3(a) * normf3(b));
    return (float)acos((double)((1.f < cs) ? 1.f : cs));
}

}  // namespace nrs
