// Host check of the per-row frame arithmetic of tfep_amd/csrc/frames.h, which is __host__ __device__: the rotation puts the
// axis point on the axis and the plane point on the plane with det R = 1, and frame_rotation_vjp agrees with central
// differences of frame_rotation, for all six (axis, plane) pairs.  Exit status 0 when every check holds.  Build and run
// (no device needed; tests/test_frames_host.py does this):
//     hipcc -std=c++17 --cuda-host-only -x hip tools/frames_host_check.cpp -o frames_host_check && ./frames_host_check
#include "../tfep_amd/csrc/frames.h"

#include <stdio.h>
#include <stdlib.h>

using namespace tfep;

static double rnd() { return 2.0 * rand() / RAND_MAX - 1.0; }

static double contract(const double (&G)[3][3], const double (&A)[3][3], const double (&B)[3][3], double h) {
    double s = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) s += G[i][j] * (A[i][j] - B[i][j]) / (2.0 * h);
    return s;
}

int main() {
    srand(7);
    double worst_vjp = 0.0, worst_geometry = 0.0;
    for (int ax = 0; ax < 3; ++ax)
        for (int pl = 0; pl < 3; ++pl) {
            if (pl == ax) continue;
            const int nn = 3 - ax - pl, sign = ((pl - ax + 3) % 3 == 1) ? 1 : -1;        // e_ax x e_pl = sign e_nn
            const FrameAxes f{ax, pl, sign * (nn + 1)};
            if (!frame_axes_valid(f)) return 2;
            for (int t = 0; t < 50; ++t) {
                double a[3] = {rnd(), rnd(), rnd()}, p[3] = {rnd(), rnd(), rnd()}, G[3][3], R[3][3];
                for (auto& row : G)
                    for (auto& v : row) v = rnd();
                FrameState st;
                frame_rotation(a, p, f, R, st);
                const double det = R[0][0] * (R[1][1] * R[2][2] - R[1][2] * R[2][1]) -
                                   R[0][1] * (R[1][0] * R[2][2] - R[1][2] * R[2][0]) +
                                   R[0][2] * (R[1][0] * R[2][1] - R[1][1] * R[2][0]);
                double ra[3], rp[3];
                for (int i = 0; i < 3; ++i) {
                    ra[i] = R[i][0] * a[0] + R[i][1] * a[1] + R[i][2] * a[2];
                    rp[i] = R[i][0] * p[0] + R[i][1] * p[1] + R[i][2] * p[2];
                }
                const double geometry = fabs(det - 1.0) + fabs(ra[pl]) + fabs(ra[nn]) + fabs(rp[nn]);
                if (geometry > worst_geometry) worst_geometry = geometry;
                double ga[3], gp[3];
                frame_rotation_vjp(p, f, st, G, ga, gp);
                for (int k = 0; k < 6; ++k) {
                    const double h = 1e-6;
                    double ap[3] = {a[0], a[1], a[2]}, am[3] = {a[0], a[1], a[2]};
                    double pp[3] = {p[0], p[1], p[2]}, pm[3] = {p[0], p[1], p[2]};
                    if (k < 3) ap[k] += h, am[k] -= h;
                    else pp[k - 3] += h, pm[k - 3] -= h;
                    double Rp[3][3], Rm[3][3];
                    FrameState unused;
                    frame_rotation(ap, pp, f, Rp, unused);
                    frame_rotation(am, pm, f, Rm, unused);
                    const double fd = contract(G, Rp, Rm, h), an = k < 3 ? ga[k] : gp[k - 3];
                    const double err = fabs(fd - an) / (1.0 + fabs(an));
                    if (err > worst_vjp) worst_vjp = err;
                }
            }
        }
    printf("worst |vjp - central difference| / (1 + |vjp|) = %.3e, worst geometry residual = %.3e\n", worst_vjp,
           worst_geometry);
    // central differences with h = 1e-6 in fp64 carry about h^2 + eps / h ~ 1e-10 per unit of curvature; the points are
    // O(1) but |a| can be small (curvature ~ 1 / |a|^2): 1e-6 leaves room for |a| down to 1e-2
    return (worst_vjp <= 1e-6 && worst_geometry <= 1e-12) ? 0 : 1;
}
