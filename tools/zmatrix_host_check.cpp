// Host check of the per-atom arithmetic of tfep_amd/csrc/zmatrix.h, which is __host__ __device__:
//   place_atom against the project's own internal coordinates (geometry.h): the distance, angle and dihedral of the
//   placed atom are the (d, a, t) it was placed with, and its log-det is 2 log d + log|sin a|;
//   place_atom_vjp against central differences, taken in long double, of the placement restated here in long double
//   from the header's comment (compared with the header's forward first), with a cotangent on the position and one on
//   the log-det.
// Exit status 0 when every check holds; a failing case is named on stderr.  Build and run (no device needed;
// tests/test_zmatrix_host.py does this):
//     hipcc -std=c++17 --cuda-host-only -x hip tools/zmatrix_host_check.cpp -o zmatrix_host_check && ./zmatrix_host_check
#include "../tfep_amd/csrc/zmatrix.h"

#include <stdio.h>

using namespace tfep;
typedef long double real;

// step 1e-5: the truncation error of a central difference is h^2 f''' / 6 = 1.7e-11 f''', and the third derivatives of
// the placement at the sets below (d <= 1.6, |x_k - x_j| >= 1, rejections >= 0.9, sin a >= 0.56) are below 100: 1e-7
// relative to the largest component of the VJP is the step squared with that margin
static const real H = 1e-5L;
static const double VJP_TOL = 1e-7, ROUND_TRIP_TOL = 1e-13, FORWARD_TOL = 1e-13;

static int failures = 0;

static void check(const char* what, int set, double err, double tol) {
    printf("%-52s set %d: %.3e (bound %.0e)\n", what, set, err, tol);
    if (!(err <= tol)) {
        fprintf(stderr, "FAILED: %s, set %d: %.3e > %.0e\n", what, set, err, tol);
        ++failures;
    }
}

// v = (d, a, t, x_j, x_k, x_l): 12 numbers; out = (x_i, log-det)
static void place_l(const real* v, real (&out)[4]) {
    const real d = v[0], a = v[1], t = v[2], *xj = v + 3, *xk = v + 6, *xl = v + 9;
    real b1[3], r[3], q[3], w[3];
    for (int c = 0; c < 3; ++c) b1[c] = xk[c] - xj[c], r[c] = xl[c] - xk[c];
    const real ne = sqrtl(b1[0] * b1[0] + b1[1] * b1[1] + b1[2] * b1[2]);
    for (int c = 0; c < 3; ++c) b1[c] /= ne;
    const real s = r[0] * b1[0] + r[1] * b1[1] + r[2] * b1[2];
    for (int c = 0; c < 3; ++c) q[c] = r[c] - s * b1[c];
    const real nq = sqrtl(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
    for (int c = 0; c < 3; ++c) w[c] = q[c] / nq;
    const real n[3] = {b1[1] * w[2] - b1[2] * w[1], b1[2] * w[0] - b1[0] * w[2], b1[0] * w[1] - b1[1] * w[0]};
    for (int c = 0; c < 3; ++c) out[c] = xj[c] + d * (cosl(a) * b1[c] + sinl(a) * (cosl(t) * w[c] - sinl(t) * n[c]));
    out[3] = 2 * logl(d) + logl(fabsl(sinl(a)));
}

// (d, a, t, x_j, x_k, x_l): the value ranges of the tests (d in [0.9, 1.6], a in [0.6, 2.5], t on both sides of 0 and
// near the cut at +-pi)
static const double SETS[][12] = {
    {1.1, 1.9, 0.7, 0.3, -0.2, 0.1, 1.4, 0.3, -0.4, 1.9, 1.5, 0.2},
    {0.9, 0.6, -2.4, -1.2, 0.7, 2.1, -0.4, 0.1, 1.3, 0.5, 0.9, 1.0},
    {1.6, 2.5, 3.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.1, -0.9, -0.5},
    {1.3, 1.2, -3.1, 2.5, -1.5, 0.5, 1.0, -1.0, 1.5, 1.2, 0.4, 2.0},
    {1.0, 1.5707963267948966, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 1.0, 0.0},
};
// cotangents of (x_i, log-det)
static const double COTANGENTS[][4] = {
    {1.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 1.0}, {0.4, -1.1, 0.8, 0.6}, {-0.7, 0.2, 1.3, -0.9}, {0.5, 0.5, -0.5, 0.3}};

int main() {
    const int n_sets = sizeof SETS / sizeof SETS[0];
    const double pi = acos(-1.0);
    for (int s = 0; s < n_sets; ++s) {
        const double* v = SETS[s];
        const double d = v[0], a = v[1], t = v[2];
        double xj[3], xk[3], xl[3], xi[3];
        for (int c = 0; c < 3; ++c) xj[c] = v[3 + c], xk[c] = v[6 + c], xl[c] = v[9 + c];
        PlaceState ps;
        const double ldj = place_atom(xj, xk, xl, d, a, t, xi, ps);

        // the inverse of the project's own conventions
        DihedralState st;
        check("ic_distance of the placed atom", s, fabs(ic_distance(xi, xj) - d), ROUND_TRIP_TOL);
        check("ic_angle of the placed atom", s, fabs(ic_angle(xi, xj, xk) - a), ROUND_TRIP_TOL);
        double dt = ic_dihedral(xi, xj, xk, xl, st) - t;
        dt -= 2.0 * pi * nearbyint(dt / (2.0 * pi));
        check("ic_dihedral of the placed atom", s, fabs(dt), ROUND_TRIP_TOL);
        check("log-det is 2 log d + log|sin a|", s, fabs(ldj - (2.0 * log(d) + log(fabs(sin(a))))), FORWARD_TOL);

        // the restatement in long double
        real q[12], ref[4];
        for (int i = 0; i < 12; ++i) q[i] = v[i];
        place_l(q, ref);
        double err = fabs(ldj - (double)ref[3]);
        for (int c = 0; c < 3; ++c) err = fmax(err, fabs(xi[c] - (double)ref[c]));
        check("place_atom against long double", s, err, FORWARD_TOL);

        // the VJP: (gd, ga, gt, g x_j, g x_k, g x_l) in the order of the inputs
        const double* g = COTANGENTS[s];
        const double gx[3] = {g[0], g[1], g[2]};
        double got[12], (&gj)[3] = *reinterpret_cast<double (*)[3]>(got + 3), (&gk)[3] = *reinterpret_cast<double (*)[3]>(got + 6),
                        (&gl)[3] = *reinterpret_cast<double (*)[3]>(got + 9);
        place_atom_vjp(xj, xk, xl, d, a, t, gx, g[3], got[0], got[1], got[2], gj, gk, gl);
        double scale = 0.0;
        err = 0.0;
        for (int i = 0; i < 12; ++i) {
            const real keep = q[i];
            real up[4], down[4], fd = 0;
            q[i] = keep + H;
            place_l(q, up);
            q[i] = keep - H;
            place_l(q, down);
            q[i] = keep;
            for (int c = 0; c < 4; ++c) fd += g[c] * (up[c] - down[c]) / (2 * H);
            scale = fmax(scale, fabs((double)fd));
            err = fmax(err, fabs(got[i] - (double)fd));
        }
        check("place_atom_vjp against central differences", s, err / scale, VJP_TOL);
        // a translation of the three references translates x_i: their cotangents sum to that of x_i
        double sum = 0.0;
        for (int c = 0; c < 3; ++c) sum = fmax(sum, fabs(gj[c] + gk[c] + gl[c] - gx[c]));
        check("reference cotangents sum to that of x_i", s, sum / scale, 1e-12);
    }
    printf("%d check(s) failed\n", failures);
    return failures ? 1 : 0;
}
