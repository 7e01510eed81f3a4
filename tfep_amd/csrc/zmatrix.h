// Placement of one atom from a Z-matrix row -- the inverse of the internal coordinates of geometry.h -- and its
// reverse-mode derivative, shared by the kernels of zmatrix.hip.  Per atom and in fp64, whatever the element type of the
// tensors (as geometry.h).
//
// A row (i, j, k, l) with values (d, a, t) places atom i from the three placed atoms j, k, l:
//   b1 = unit(x_k - x_j)
//   w  = unit((x_l - x_k) - ((x_l - x_k) . b1) b1)             the rejection of x_l - x_k from b1
//   n  = b1 x w
//   x_i = x_j + d (cos a  b1 + sin a (cos t  w - sin t  n))
// so that ic_distance(x_i, x_j) = d, ic_angle(x_i, x_j, x_k) = a and ic_dihedral(x_i, x_j, x_k, x_l) = t for d > 0,
// a in (0, pi), t in (-pi, pi]: b1, w, n is a right-handed orthonormal frame with b1 x n = -w, the rejection of
// x_i - x_j from b1 is d sin a (cos t  w - sin t  n) and b1 x that is d sin a (cos t  n + sin t  w), whose products with w
// are d sin a cos t and d sin a sin t (tools/zmatrix_host_check.cpp checks the three identities numerically).
//
// The Jacobian of (d, a, t) -> x_i is d^2 |sin a| (spherical coordinates about x_j in the frame above), so one placed
// atom contributes 2 log d + log|sin a| to the log-det; the whole map is block triangular in placement order.
//
// Degenerate geometry is not special-cased: collinear j, k, l (a zero rejection), coincident j, k or d = 0 divide by zero
// and give NaN or infinite values and cotangents, as geometry.h does.
#pragma once
#include "geometry.h"

namespace tfep {

// What the placement's derivative needs of its forward.
struct PlaceState {
    double b1[3], w[3], n[3], r[3], ne, nq, s, ca, sa, ct, st;
};

// x_i from the three reference positions and (d, a, t); returns the atom's log-det contribution.
__host__ __device__ inline double place_atom(const double (&xj)[3], const double (&xk)[3], const double (&xl)[3], double d,
                                             double a, double t, double (&xi)[3], PlaceState& ps) {
    double e[3], q[3];
    sub3(xk, xj, e);
    sub3(xl, xk, ps.r);
    ps.ne = sqrt(dot3(e, e));
#pragma unroll
    for (int c = 0; c < 3; ++c) ps.b1[c] = e[c] / ps.ne;
    ps.s = dot3(ps.r, ps.b1);
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = ps.r[c] - ps.s * ps.b1[c];
    ps.nq = sqrt(dot3(q, q));
#pragma unroll
    for (int c = 0; c < 3; ++c) ps.w[c] = q[c] / ps.nq;
    cross3(ps.b1, ps.w, ps.n);
    ps.ca = cos(a), ps.sa = sin(a), ps.ct = cos(t), ps.st = sin(t);
#pragma unroll
    for (int c = 0; c < 3; ++c)
        xi[c] = xj[c] + d * (ps.ca * ps.b1[c] + ps.sa * (ps.ct * ps.w[c] - ps.st * ps.n[c]));
    return 2.0 * log(d) + log(fabs(ps.sa));
}

// Cotangents of (d, a, t) and of the three reference positions from the cotangent g of x_i and gl of the log-det.
__host__ __device__ inline void place_atom_vjp(const double (&xj)[3], const double (&xk)[3], const double (&xl)[3], double d,
                                               double a, double t, const double (&g)[3], double gl, double& gd, double& ga,
                                               double& gt, double (&gj)[3], double (&gk)[3], double (&gl3)[3]) {
    PlaceState ps;
    double xi[3];
    place_atom(xj, xk, xl, d, a, t, xi, ps);
    // x_i = x_j + d (ca b1 + sa p),  p = ct w - st n
    const double gb = dot3(g, ps.b1), gw_ = dot3(g, ps.w), gn_ = dot3(g, ps.n);
    gd = ps.ca * gb + ps.sa * (ps.ct * gw_ - ps.st * gn_) + 2.0 * gl / d;
    ga = d * (-ps.sa * gb + ps.ca * (ps.ct * gw_ - ps.st * gn_)) + gl * ps.ca / ps.sa;
    gt = -d * ps.sa * (ps.st * gw_ + ps.ct * gn_);
    double gb1[3], gw[3], gn[3], t0[3], t1[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        gb1[c] = d * ps.ca * g[c];
        gw[c] = d * ps.sa * ps.ct * g[c];
        gn[c] = -d * ps.sa * ps.st * g[c];
    }
    // n = b1 x w
    cross3(ps.w, gn, t0);
    cross3(gn, ps.b1, t1);
#pragma unroll
    for (int c = 0; c < 3; ++c) gb1[c] += t0[c], gw[c] += t1[c];
    // w = q / |q|,  q = r - (r . b1) b1,  r = x_l - x_k
    const double dw = dot3(gw, ps.w);
    double gq[3], gr[3], ge[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) gq[c] = (gw[c] - dw * ps.w[c]) / ps.nq;
    const double dq = dot3(gq, ps.b1);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        gr[c] = gq[c] - dq * ps.b1[c];
        gb1[c] += -ps.s * gq[c] - dq * ps.r[c];
    }
    // b1 = e / |e|,  e = x_k - x_j
    const double d1 = dot3(gb1, ps.b1);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        ge[c] = (gb1[c] - d1 * ps.b1[c]) / ps.ne;
        gj[c] = g[c] - ge[c];
        gk[c] = ge[c] - gr[c];
        gl3[c] = gr[c];
    }
}

}  // namespace tfep
