// Host check of the per-entry arithmetic of tfep_amd/csrc/geometry.h, which is __host__ __device__: the four hand-derived
// VJPs (ic_distance_vjp, ic_angle_vjp, ic_dihedral_vjp, polar_map_vjp in both directions) against central differences of
// the forward maps, on a few fixed well-conditioned point sets.  The differences are taken in long double, of the forward
// maps restated here in long double from the header's comment (the fp64 forwards carry eps / h = 1e-11 of noise at this
// step, and a restatement is a second opinion on them: it is compared with the header's forwards first).  Exit status 0
// when every check holds; a failing case is named on stderr.  Build and run (no device needed;
// tests/test_geometry_host.py does this):
//     hipcc -std=c++17 --cuda-host-only -x hip tools/geometry_host_check.cpp -o geometry_host_check && ./geometry_host_check
#include "../tfep_amd/csrc/geometry.h"

#include <stdio.h>

using namespace tfep;
typedef long double real;

// step 1e-5: the truncation error of a central difference is h^2 f''' / 6 = 1.7e-11 f''', and the third derivatives of
// these maps at the points below (distances >= 1, sin(angle) >= 0.89, rejections >= 0.98) are below 100: 1e-7 relative
// to the largest component of the VJP is the step squared with that margin
static const real H = 1e-5L;
static const double VJP_TOL = 1e-7, FORWARD_TOL = 1e-13, SUM_TOL = 1e-12;

static int failures = 0;

static void check(const char* what, int set, double err, double tol) {
    printf("%-44s set %d: %.3e (bound %.0e)\n", what, set, err, tol);
    if (!(err <= tol)) {
        fprintf(stderr, "FAILED: %s, point set %d: %.3e > %.0e\n", what, set, err, tol);
        ++failures;
    }
}

// ------------------------------------------------------------------------------------------ the forwards in long double

static real dotl(const real* a, const real* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

static real distance_l(const real* p) {          // p: 2 points
    const real r[3] = {p[3] - p[0], p[4] - p[1], p[5] - p[2]};
    return sqrtl(dotl(r, r));
}

static real angle_l(const real* p) {             // p: 3 points, the angle at the middle one
    real u[3], v[3];
    for (int c = 0; c < 3; ++c) u[c] = p[c] - p[3 + c], v[c] = p[6 + c] - p[3 + c];
    const real cs = dotl(u, v) / (sqrtl(dotl(u, u)) * sqrtl(dotl(v, v)));
    return acosl(cs < -1 ? -1 : cs > 1 ? 1 : cs);
}

static real dihedral_l(const real* p) {          // p: 4 points
    real b0[3], b1[3], b2[3], v[3], w[3];
    for (int c = 0; c < 3; ++c) b0[c] = p[c] - p[3 + c], b1[c] = p[6 + c] - p[3 + c], b2[c] = p[9 + c] - p[6 + c];
    const real ne = sqrtl(dotl(b1, b1));
    for (int c = 0; c < 3; ++c) b1[c] /= ne;
    const real s0 = dotl(b0, b1), s2 = dotl(b2, b1);
    for (int c = 0; c < 3; ++c) v[c] = b0[c] - s0 * b1[c], w[c] = b2[c] - s2 * b1[c];
    const real m[3] = {b1[1] * v[2] - b1[2] * v[1], b1[2] * v[0] - b1[0] * v[2], b1[0] * v[1] - b1[1] * v[0]};
    return atan2l(dotl(m, w), dotl(v, w));
}

static void polar_l(int to_cartesian, real a, real b, real (&o)[3]) {
    if (to_cartesian) {
        o[0] = a * cosl(b), o[1] = a * sinl(b), o[2] = logl(a);
    } else {
        o[0] = sqrtl(a * a + b * b), o[1] = atan2l(b, a), o[2] = -logl(o[0]);
    }
}

// ------------------------------------------------------------------------------------------ the checks

// g * d f / d p by central differences, for the n_points points of `p`
template <typename F>
static void central(F f, const double* p, int n_points, double g, double* out) {
    real q[12];
    for (int i = 0; i < 3 * n_points; ++i) q[i] = p[i];
    for (int i = 0; i < 3 * n_points; ++i) {
        const real keep = q[i];
        q[i] = keep + H;
        const real up = f(q);
        q[i] = keep - H;
        const real down = f(q);
        q[i] = keep;
        real diff = up - down;                       // (a dihedral may cross the cut at +-pi between the two)
        const real pi = acosl(-1.0L);
        if (diff > pi) diff -= 2 * pi;
        if (diff < -pi) diff += 2 * pi;
        out[i] = (double)(g * diff / (2 * H));
    }
}

// the largest component error relative to the largest component, and the sum of the point cotangents likewise
static void compare(const char* what, int set, const double* got, const double* fd, int n_points) {
    double scale = 0.0, err = 0.0, sum[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < 3 * n_points; ++i) {
        scale = fmax(scale, fabs(fd[i]));
        err = fmax(err, fabs(got[i] - fd[i]));
        sum[i % 3] += got[i];
    }
    char name[96];
    snprintf(name, sizeof name, "%s against central differences", what);
    check(name, set, err / scale, VJP_TOL);
    snprintf(name, sizeof name, "%s cotangents sum to zero", what);
    check(name, set, fmax(fabs(sum[0]), fmax(fabs(sum[1]), fabs(sum[2]))) / scale, SUM_TOL);
}

// four points per set: the first two serve the distance, the first three the angle
static const double POINTS[][12] = {
    {0.3, -0.2, 0.1, 1.4, 0.3, -0.4, 1.9, 1.5, 0.2, 3.1, 1.7, 1.3},            // a bent chain
    {-1.2, 0.7, 2.1, -0.4, 0.1, 1.3, 0.5, 0.9, 1.0, 0.8, 2.2, 0.1},           // a negative dihedral, -1.31
    {0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.1, 0.0, 0.0, 1.3, -0.9, -0.5},           // dihedral -2.63
    {2.5, -1.5, 0.5, 1.0, -1.0, 1.5, 1.2, 0.4, 2.0, -0.3, 0.9, 2.6},           // dihedral 2.94, 0.2 from the cut
};
static const double COTANGENTS[] = {1.0, -0.7, 1.3, 0.45};
// (a, b) of the polar maps: Cartesian points in all four quadrants, which also serve as (r > 0, angle)
static const double PLANE[][2] = {{1.3, 0.4}, {0.7, -2.1}, {2.2, 2.9}, {0.6, -0.3}, {-1.1, 0.8}, {-0.9, -1.7}};
static const double PLANE_COTANGENTS[][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}, {0.8, -1.1, 0.6}};

template <int K>
static void as_points(const double* p, double (&out)[K][3]) {
    for (int i = 0; i < K; ++i)
        for (int c = 0; c < 3; ++c) out[i][c] = p[3 * i + c];
}

int main() {
    const int n_sets = sizeof POINTS / sizeof POINTS[0];
    for (int s = 0; s < n_sets; ++s) {
        const double g = COTANGENTS[s];
        double p[4][3], got[12], fd[12];
        real q[12];
        as_points<4>(POINTS[s], p);
        for (int i = 0; i < 12; ++i) q[i] = POINTS[s][i];

        check("ic_distance against long double", s, fabs(ic_distance(p[0], p[1]) - (double)distance_l(q)), FORWARD_TOL);
        double (&g2)[2][3] = *reinterpret_cast<double (*)[2][3]>(got);
        ic_distance_vjp(p[0], p[1], g, g2[0], g2[1]);
        central(distance_l, POINTS[s], 2, g, fd);
        compare("ic_distance_vjp", s, got, fd, 2);

        check("ic_angle against long double", s, fabs(ic_angle(p[0], p[1], p[2]) - (double)angle_l(q)), FORWARD_TOL);
        double (&g3)[3][3] = *reinterpret_cast<double (*)[3][3]>(got);
        ic_angle_vjp(p[0], p[1], p[2], g, g3[0], g3[1], g3[2]);
        central(angle_l, POINTS[s], 3, g, fd);
        compare("ic_angle_vjp", s, got, fd, 3);

        DihedralState st;
        check("ic_dihedral against long double", s, fabs(ic_dihedral(p[0], p[1], p[2], p[3], st) - (double)dihedral_l(q)),
              FORWARD_TOL);
        double (&g4)[4][3] = *reinterpret_cast<double (*)[4][3]>(got);
        ic_dihedral_vjp(p[0], p[1], p[2], p[3], g, g4[0], g4[1], g4[2], g4[3]);
        central(dihedral_l, POINTS[s], 4, g, fd);
        compare("ic_dihedral_vjp", s, got, fd, 4);
    }

    const int n_plane = sizeof PLANE / sizeof PLANE[0], n_cot = sizeof PLANE_COTANGENTS / sizeof PLANE_COTANGENTS[0];
    for (int to_cartesian = 0; to_cartesian < 2; ++to_cartesian)
        for (int s = 0; s < n_plane; ++s) {
            const double a = to_cartesian ? fabs(PLANE[s][0]) : PLANE[s][0], b = PLANE[s][1];
            const char* name = to_cartesian ? "polar_map_vjp to Cartesian" : "polar_map_vjp to polar";
            double o0, o1, ol;
            real ref[3];
            polar_map(to_cartesian, a, b, o0, o1, ol);
            polar_l(to_cartesian, a, b, ref);
            check(to_cartesian ? "polar_map to Cartesian against long double" : "polar_map to polar against long double", s,
                  fmax(fabs(o0 - (double)ref[0]), fmax(fabs(o1 - (double)ref[1]), fabs(ol - (double)ref[2]))), FORWARD_TOL);
            double err = 0.0, scale = 0.0;
            for (int k = 0; k < n_cot; ++k) {
                const double* g = PLANE_COTANGENTS[k];
                double ga, gb;
                polar_map_vjp(to_cartesian, a, b, g[0], g[1], g[2], ga, gb);
                for (int i = 0; i < 2; ++i) {
                    real up[3], down[3];
                    polar_l(to_cartesian, a + (i == 0 ? H : 0), b + (i == 1 ? H : 0), up);
                    polar_l(to_cartesian, a - (i == 0 ? H : 0), b - (i == 1 ? H : 0), down);
                    real fd = 0;
                    for (int c = 0; c < 3; ++c) fd += g[c] * (up[c] - down[c]) / (2 * H);
                    scale = fmax(scale, fabs((double)fd));
                    err = fmax(err, fabs((i == 0 ? ga : gb) - (double)fd));
                }
            }
            check(name, s, err / scale, VJP_TOL);
        }
    printf("%d check(s) failed\n", failures);
    return failures ? 1 : 0;
}
