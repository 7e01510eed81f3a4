// Internal coordinates of a row of points -- distance, angle, proper dihedral -- and their reverse-mode derivatives
// (reference utils/geometry.py:28-178), and the polar map of the plane (geometry.py:414-471), shared by the kernels of
// geometry.hip.  Everything is per entry and in fp64, whatever the element type of the tensors (as frames.h): a float32
// row is widened on load and rounded once on store.
//
// The formulations are the reference's, step by step, so that signs, branches and degenerate values agree:
//   distance  |p1 - p0|                                             (0 for coincident points)
//   angle     acos(clamp(u . v / (|u| |v|), -1, 1)),  u = p0 - p1, v = p2 - p1
//   dihedral  b0 = p0 - p1, b1 = (p2 - p1) / |p2 - p1|, b2 = p3 - p2; the rejections v = b0 - (b0 . b1) b1 and
//             w = b2 - (b2 . b1) b1;  atan2((b1 x v) . w, v . w)     (atan2(0, 0) = 0 for a collinear quad)
// Degenerate geometry is not special-cased in the derivatives either: coincident or collinear points divide by zero
// and the cotangents are NaN or infinite, as autograd gives them for the torch code.  Outside the clamp the angle has
// zero derivative, on its boundary the derivative of acos is infinite: both as torch.clamp / torch.acos have it.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace tfep {

__host__ __device__ inline double dot3(const double (&a)[3], const double (&b)[3]) {
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}
__host__ __device__ inline void sub3(const double (&a)[3], const double (&b)[3], double (&c)[3]) {
    c[0] = a[0] - b[0], c[1] = a[1] - b[1], c[2] = a[2] - b[2];
}
__host__ __device__ inline void cross3(const double (&a)[3], const double (&b)[3], double (&c)[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1], c[1] = a[2] * b[0] - a[0] * b[2], c[2] = a[0] * b[1] - a[1] * b[0];
}

__host__ __device__ inline double ic_distance(const double (&p0)[3], const double (&p1)[3]) {
    double r[3];
    sub3(p1, p0, r);
    return sqrt(dot3(r, r));
}

// Cotangents of the two points from the cotangent g of the distance.
__host__ __device__ inline void ic_distance_vjp(const double (&p0)[3], const double (&p1)[3], double g,
                                                double (&g0)[3], double (&g1)[3]) {
    double r[3];
    sub3(p1, p0, r);
    const double s = g / sqrt(dot3(r, r));
#pragma unroll
    for (int c = 0; c < 3; ++c) g1[c] = s * r[c], g0[c] = -g1[c];
}

__host__ __device__ inline double ic_angle(const double (&p0)[3], const double (&p1)[3], const double (&p2)[3]) {
    double u[3], v[3];
    sub3(p0, p1, u);
    sub3(p2, p1, v);
    const double c = dot3(u, v) / (sqrt(dot3(u, u)) * sqrt(dot3(v, v)));
    return acos(c < -1.0 ? -1.0 : c > 1.0 ? 1.0 : c);      // (a NaN cosine stays NaN)
}

__host__ __device__ inline void ic_angle_vjp(const double (&p0)[3], const double (&p1)[3], const double (&p2)[3], double g,
                                             double (&g0)[3], double (&g1)[3], double (&g2)[3]) {
    double u[3], v[3];
    sub3(p0, p1, u);
    sub3(p2, p1, v);
    const double nu = sqrt(dot3(u, u)), nv = sqrt(dot3(v, v)), c = dot3(u, v) / (nu * nv);
    const double gc = (c < -1.0 || c > 1.0) ? 0.0 : -g / sqrt(1.0 - c * c);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        g0[k] = gc * (v[k] / (nu * nv) - c * u[k] / (nu * nu));
        g2[k] = gc * (u[k] / (nu * nv) - c * v[k] / (nv * nv));
        g1[k] = -(g0[k] + g2[k]);
    }
}

// What the dihedral's derivative needs of its forward.
struct DihedralState {
    double b0[3], b1[3], b2[3], ne, s0, s2, v[3], w[3], m[3], x, y;
};

__host__ __device__ inline double ic_dihedral(const double (&p0)[3], const double (&p1)[3], const double (&p2)[3],
                                              const double (&p3)[3], DihedralState& st) {
    double e[3];
    sub3(p0, p1, st.b0);
    sub3(p2, p1, e);
    sub3(p3, p2, st.b2);
    st.ne = sqrt(dot3(e, e));
#pragma unroll
    for (int c = 0; c < 3; ++c) st.b1[c] = e[c] / st.ne;
    st.s0 = dot3(st.b0, st.b1);
    st.s2 = dot3(st.b2, st.b1);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        st.v[c] = st.b0[c] - st.s0 * st.b1[c];
        st.w[c] = st.b2[c] - st.s2 * st.b1[c];
    }
    st.x = dot3(st.v, st.w);
    cross3(st.b1, st.v, st.m);
    st.y = dot3(st.m, st.w);
    return atan2(st.y, st.x);
}

__host__ __device__ inline void ic_dihedral_vjp(const double (&p0)[3], const double (&p1)[3], const double (&p2)[3],
                                                const double (&p3)[3], double g, double (&g0)[3], double (&g1)[3],
                                                double (&g2)[3], double (&g3)[3]) {
    DihedralState st;
    ic_dihedral(p0, p1, p2, p3, st);
    // t = atan2(y, x)
    const double r2 = st.x * st.x + st.y * st.y, gx = -st.y / r2 * g, gy = st.x / r2 * g;
    // x = v . w,  y = m . w,  m = b1 x v
    double gv[3], gw[3], gm[3], gb1[3], t[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        gw[c] = gx * st.v[c] + gy * st.m[c];
        gm[c] = gy * st.w[c];
    }
    cross3(st.v, gm, gb1);
    cross3(gm, st.b1, t);
#pragma unroll
    for (int c = 0; c < 3; ++c) gv[c] = gx * st.w[c] + t[c];
    // v = b0 - (b0 . b1) b1,  w = b2 - (b2 . b1) b1
    const double dv = dot3(gv, st.b1), dw = dot3(gw, st.b1);
    double gb0[3], gb2[3], ge[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        gb0[c] = gv[c] - dv * st.b1[c];
        gb2[c] = gw[c] - dw * st.b1[c];
        gb1[c] += -dv * st.b0[c] - st.s0 * gv[c] - dw * st.b2[c] - st.s2 * gw[c];
    }
    // b1 = e / |e|,  e = p2 - p1;  b0 = p0 - p1;  b2 = p3 - p2
    const double d1 = dot3(gb1, st.b1);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        ge[c] = (gb1[c] - d1 * st.b1[c]) / st.ne;
        g0[c] = gb0[c];
        g1[c] = -gb0[c] - ge[c];
        g2[c] = ge[c] - gb2[c];
        g3[c] = gb2[c];
    }
}

// The polar map of the plane and its inverse, with the log-det the reference returns with each (minus, plus log r).
//   to_cartesian == 0: (x, y) -> (r, angle) = (sqrt(x^2 + y^2), atan2(y, x)),  log_det_J = -log r
//   to_cartesian != 0: (r, angle) -> (x, y) = (r cos, r sin),                  log_det_J = +log r
__host__ __device__ inline void polar_map(int to_cartesian, double a, double b, double& o0, double& o1, double& ldj) {
    if (to_cartesian) {
        o0 = a * cos(b), o1 = a * sin(b), ldj = log(a);
    } else {
        o0 = sqrt(a * a + b * b), o1 = atan2(b, a), ldj = -log(o0);
    }
}

// Cotangents (ga, gb) of the two inputs from those of the two outputs and of the log-det.
__host__ __device__ inline void polar_map_vjp(int to_cartesian, double a, double b, double g0, double g1, double gl,
                                              double& ga, double& gb) {
    if (to_cartesian) {
        const double c = cos(b), s = sin(b);
        ga = g0 * c + g1 * s + gl / a;
        gb = a * (g1 * c - g0 * s);
    } else {
        const double r2 = a * a + b * b, r = sqrt(r2);
        ga = g0 * a / r - g1 * b / r2 - gl * a / r2;
        gb = g0 * b / r + g1 * a / r2 - gl * b / r2;
    }
}

}  // namespace tfep
