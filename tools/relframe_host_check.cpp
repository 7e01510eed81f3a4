// Host check of the per-row arithmetic of tfep_amd/csrc/relframe.h, which is __host__ __device__: the very functions the
// kernels of relframe.hip call, run here with the lanes of a wave played by a loop.  For n_c = 5 atoms and all 8 settings of
// `remove`: decode(encode(x)) = x with log-dets that cancel; the hand-written VJPs of encode and of decode agree with central
// differences of sum(cotangent * output); and a row whose axis vector is exactly (-2, 0, 0) takes the rotation by pi, a proper
// rotation that puts the axis atom at (2, 0, 0).  Exit status 0 when every check holds.  Build and run (no device needed;
// tests/test_relframe_host.py does this, with -fsanitize=address,undefined):
//     hipcc -std=c++17 --cuda-host-only -x hip tools/relframe_host_check.cpp -o relframe_host_check && ./relframe_host_check
#include "../tfep_amd/csrc/relframe.h"

#include <stdio.h>
#include <stdlib.h>

#include <vector>

using namespace tfep;

constexpr int N_C = 5, LANES = 2;        // two "lanes": the partial sums of the VJPs are added up as wave_sum does
constexpr int NX = 3 * N_C;

static double rnd() { return 2.0 * rand() / RAND_MAX - 1.0; }

struct Encoded {
    std::vector<double> coords;
    double origin[3], rot[9], ldj;
};

static Encoded encode(const double* x, const RelRemove& rm) {
    Encoded e;
    e.coords.assign(relframe_width(N_C, rm), 0.0);
    for (int lane = 0; lane < LANES; ++lane) relframe_encode_row(x, N_C, rm, lane, LANES, e.coords.data(), e.origin, e.rot, &e.ldj);
    return e;
}

static void decode(const Encoded& e, const RelRemove& rm, double* x, double* ldj) {
    for (int lane = 0; lane < LANES; ++lane)
        relframe_decode_row(e.coords.data(), e.origin, e.rot, N_C, rm, lane, LANES, x, ldj);
}

// sum(cotangent * output) of encode: cot holds W + 3 + 9 + 1 values
static double encode_loss(const double* x, const RelRemove& rm, const std::vector<double>& cot) {
    const Encoded e = encode(x, rm);
    const int W = (int)e.coords.size();
    double s = cot[W + 12] * e.ldj;
    for (int k = 0; k < W; ++k) s += cot[k] * e.coords[k];
    for (int k = 0; k < 3; ++k) s += cot[W + k] * e.origin[k];
    for (int k = 0; k < 9; ++k) s += cot[W + 3 + k] * e.rot[k];
    return s;
}

// sum(cotangent * output) of decode: cot holds NX + 1 values
static double decode_loss(const Encoded& e, const RelRemove& rm, const std::vector<double>& cot) {
    double x[NX], ldj;
    decode(e, rm, x, &ldj);
    double s = cot[NX] * ldj;
    for (int k = 0; k < NX; ++k) s += cot[k] * x[k];
    return s;
}

static void note(double fd, double an, double& worst) {
    const double err = fabs(fd - an) / (1.0 + fabs(an));
    if (!(err <= worst)) worst = err;              // (a NaN sticks)
}

int main() {
    srand(11);
    const double h = 1e-6;
    double worst_vjp = 0.0, worst_round_trip = 0.0;
    int rows = 0, negative_c = 0;
    for (int mask = 0; mask < 8; ++mask) {
        const RelRemove rm{mask & 1, (mask >> 1) & 1, (mask >> 2) & 1};
        const int W = (int)relframe_width(N_C, rm);
        for (int t = 0; t < 40; ++t) {
            double x[NX];
            for (auto& v : x) v = 1.5 * rnd();
            RelFrameRow f;
            relframe_load(x, N_C, f);
            const Encoded e = encode(x, rm);
            const double c = f.da[0] / f.st.na, a102 = RELFRAME_TWO_PI * e.coords[2] - RELFRAME_PI;
            // the conditions of a row: away from the antiparallel axis, from d02 = 0 and from the cut of atan2
            if (f.st.na < 0.3 || e.coords[1] < 0.3 || 1.0 + c < 0.05 || fabs(a102) > RELFRAME_PI - 0.2) continue;
            ++rows;
            negative_c += c < -0.2;
            // the round trip (removed DOFs are zero in the frame up to round-off, so every setting inverts)
            double xb[NX], ldj_back;
            decode(e, rm, xb, &ldj_back);
            for (int k = 0; k < NX; ++k)
                if (!(fabs(xb[k] - x[k]) <= worst_round_trip)) worst_round_trip = fabs(xb[k] - x[k]);
            if (!(fabs(e.ldj + ldj_back) <= worst_round_trip)) worst_round_trip = fabs(e.ldj + ldj_back);

            // encode's VJP
            std::vector<double> cot(W + 13);
            for (auto& v : cot) v = rnd();
            double gx[NX], acc[12] = {0.0}, part[12];
            for (int lane = 0; lane < LANES; ++lane) {
                relframe_encode_vjp_atoms(x, N_C, f, cot.data(), lane, LANES, gx, part);
                for (int k = 0; k < 12; ++k) acc[k] += part[k];
            }
            relframe_encode_vjp_refs(N_C, rm, f, cot.data(), cot.data() + W, cot.data() + W + 3, cot.data() + W + 12, acc, gx);
            for (int k = 0; k < NX; ++k) {
                double xp[NX], xm[NX];
                for (int j = 0; j < NX; ++j) xp[j] = xm[j] = x[j];
                xp[k] += h, xm[k] -= h;
                note((encode_loss(xp, rm, cot) - encode_loss(xm, rm, cot)) / (2.0 * h), gx[k], worst_vjp);
            }

            // decode's VJP, at coordinates whose kept DOFs are not zero and a rotation that is any matrix near R
            Encoded d = e;
            for (int k = 3 + 3 * (N_C - 3); k < W; ++k) d.coords[k] = 0.3 * rnd();
            for (auto& v : d.rot) v += 0.1 * rnd();
            std::vector<double> dcot(NX + 1);
            for (auto& v : dcot) v = rnd();
            std::vector<double> gc(W);
            double g_origin[3], g_rot[9], dacc[12] = {0.0};
            RelDecodeRow df;
            relframe_decode_load(d.coords.data(), d.origin, d.rot, N_C, rm, df);
            for (int lane = 0; lane < LANES; ++lane) {
                relframe_decode_vjp_atoms(d.coords.data(), N_C, df, dcot.data(), lane, LANES, gc.data(), part);
                for (int k = 0; k < 12; ++k) dacc[k] += part[k];
            }
            relframe_decode_vjp_refs(N_C, rm, df, dcot.data(), dcot.data() + NX, dacc, gc.data(), g_origin, g_rot);
            for (int k = 0; k < W + 12; ++k) {
                Encoded p = d, m = d;
                double* vp = k < W ? &p.coords[k] : k < W + 3 ? &p.origin[k - W] : &p.rot[k - W - 3];
                double* vm = k < W ? &m.coords[k] : k < W + 3 ? &m.origin[k - W] : &m.rot[k - W - 3];
                *vp += h, *vm -= h;
                const double an = k < W ? gc[k] : k < W + 3 ? g_origin[k - W] : g_rot[k - W - 3];
                note((decode_loss(p, rm, dcot) - decode_loss(m, rm, dcot)) / (2.0 * h), an, worst_vjp);
            }
        }
    }

    // the rotation by pi
    const double xpi[NX] = {0.3, -0.7, 1.1, -0.4, 0.9, 0.2, 0.5, -0.25, 1.0, -1.5, -0.25, 1.0, 1.25, 0.5, -0.5};
    RelFrameRow f;
    relframe_load(xpi, N_C, f);
    double worst_pi = f.st.antiparallel ? 0.0 : 1.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0.0;
            for (int k = 0; k < 3; ++k) s += f.R[i][k] * f.R[j][k];
            worst_pi = fmax(worst_pi, fabs(s - (i == j)));
        }
    const double det = f.R[0][0] * (f.R[1][1] * f.R[2][2] - f.R[1][2] * f.R[2][1]) -
                       f.R[0][1] * (f.R[1][0] * f.R[2][2] - f.R[1][2] * f.R[2][0]) +
                       f.R[0][2] * (f.R[1][0] * f.R[2][1] - f.R[1][1] * f.R[2][0]);
    const Encoded epi = encode(xpi, RelRemove{0, 0, 0});
    worst_pi = fmax(worst_pi, fabs(det - 1.0));
    worst_pi = fmax(worst_pi, fabs(epi.coords[0] - 2.0));
    for (int k = 3 + 3 * (N_C - 3); k < (int)epi.coords.size(); ++k) worst_pi = fmax(worst_pi, fabs(epi.coords[k]));

    printf("%d rows (%d with c < -0.2): worst |vjp - central difference| / (1 + |vjp|) = %.3e, worst round trip = %.3e, "
           "worst residual of the rotation by pi = %.3e\n", rows, negative_c, worst_vjp, worst_round_trip, worst_pi);
    // central differences with h = 1e-6 in fp64 carry about h^2 + eps / h ~ 1e-10 per unit of curvature: the bound of
    // tools/frames_host_check.cpp
    return (rows >= 100 && negative_c >= 10 && worst_vjp <= 1e-6 && worst_round_trip <= 1e-12 && worst_pi <= 1e-14) ? 0 : 1;
}
