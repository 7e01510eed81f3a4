// Host check of the argument checks of tfep_amd/csrc/edge_ops.hip: every entry point called with NULL pointers, negative
// sizes and empty inputs must return its code (TFEP_ERR_INVALID_ARGUMENT, or TFEP_OK for a no-op) before it launches
// anything, so none of these calls needs a device.  The source is included as it is; the two helpers it takes from
// transformers.hip (the last-error string) are restated here.  Exit status 0 when every check holds.  Build and run
// (tests/test_edge_ops_host.py does this, with -Xarch_host -fsanitize=address,undefined):
//     hipcc -std=c++17 --offload-arch=gfx950 -x hip tools/edge_ops_host_check.cpp -o edge_ops_host_check && ./edge_ops_host_check
#include "../tfep_amd/csrc/edge_ops.hip"

#include <stdarg.h>
#include <string.h>

namespace tfep {
std::string& last_error() {
    static thread_local std::string e;
    return e;
}
int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    last_error() = buf;
    return code;
}
}  // namespace tfep

static int failures = 0;

static void expect(const char* what, long long got, long long want, const char* message = nullptr) {
    const bool ok = got == want && (!message || strstr(tfep::last_error().c_str(), message));
    if (!ok) {
        printf("FAILED %s: returned %lld (expected %lld), last error '%s'\n", what, got, want, tfep::last_error().c_str());
        ++failures;
    }
    tfep::last_error().clear();
}

int main() {
    const int BAD = TFEP_ERR_INVALID_ARGUMENT;
    // host memory stands in for the tensors: no call below may reach a launch, so none of it is read
    float xf[6] = {0}, rf[2] = {0}, df[6] = {0}, gxf[6] = {0};
    double xd[6] = {0}, rd[2] = {0}, dd[6] = {0}, gxd[6] = {0};
    int64_t edges[4] = {0, 1, 1, 0}, node_ptr[3] = {0, 2, 4}, incident[4] = {0, 3, 1, 2}, ws[2] = {7, 7}, keep[2] = {0}, out[4];

    // geometry: sizes, then no-ops, then pointers and strides
    expect("geometry E < 0", tfep_edge_geometry(xf, 3, edges, 2, -1, 0, 0, rf, df, nullptr), BAD, "negative size");
    expect("geometry N < 0", tfep_edge_geometry_f64(xd, 3, edges, -2, 2, 0, 0, rd, dd, nullptr), BAD, "negative size");
    expect("geometry E too large", tfep_edge_geometry(xf, 3, edges, 2, INT64_MAX, 0, 0, rf, df, nullptr), BAD, "too many");
    expect("geometry E = 0", tfep_edge_geometry(nullptr, 0, nullptr, 2, 0, 1, 1, nullptr, nullptr, nullptr), TFEP_OK);
    expect("geometry E = 0, N = 0", tfep_edge_geometry_f64(nullptr, 0, nullptr, 0, 0, 0, 0, nullptr, nullptr, nullptr), TFEP_OK);
    expect("geometry edges without nodes", tfep_edge_geometry(xf, 3, edges, 0, 2, 0, 0, rf, df, nullptr), BAD, "without nodes");
    expect("geometry x NULL", tfep_edge_geometry(nullptr, 3, edges, 2, 2, 0, 0, rf, df, nullptr), BAD, "null tensor");
    expect("geometry edges NULL", tfep_edge_geometry_f64(xd, 3, nullptr, 2, 2, 0, 0, rd, dd, nullptr), BAD, "null tensor");
    expect("geometry distances NULL", tfep_edge_geometry(xf, 3, edges, 2, 2, 0, 0, nullptr, df, nullptr), BAD, "null tensor");
    expect("geometry directions NULL", tfep_edge_geometry_f64(xd, 3, edges, 2, 2, 0, 0, rd, nullptr, nullptr), BAD, "null tensor");
    expect("geometry ldx < 3", tfep_edge_geometry(xf, 2, edges, 2, 2, 0, 0, rf, df, nullptr), BAD, "row stride");

    // backward
    expect("backward E < 0", tfep_edge_geometry_backward(xf, 3, edges, 2, -1, node_ptr, incident, 0, 0, rf, df, gxf, 3, nullptr), BAD,
           "negative size");
    expect("backward N < 0", tfep_edge_geometry_backward_f64(xd, 3, edges, -1, 2, node_ptr, incident, 0, 0, rd, dd, gxd, 3, nullptr),
           BAD, "negative size");
    expect("backward N = 0", tfep_edge_geometry_backward(nullptr, 0, nullptr, 0, 0, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr,
                                                        0, nullptr), TFEP_OK);
    expect("backward gx NULL", tfep_edge_geometry_backward(xf, 3, edges, 2, 2, node_ptr, incident, 0, 0, rf, df, nullptr, 3, nullptr),
           BAD, "null output");
    expect("backward ldgx < 3", tfep_edge_geometry_backward_f64(xd, 3, edges, 2, 2, node_ptr, incident, 0, 0, rd, dd, gxd, 1, nullptr),
           BAD, "row stride");
    expect("backward x NULL", tfep_edge_geometry_backward(nullptr, 3, edges, 2, 2, node_ptr, incident, 0, 0, rf, df, gxf, 3, nullptr),
           BAD, "null tensor");
    expect("backward node_ptr NULL", tfep_edge_geometry_backward_f64(xd, 3, edges, 2, 2, nullptr, incident, 1, 0, rd, dd, gxd, 3,
                                                                    nullptr), BAD, "null tensor");
    expect("backward incident NULL", tfep_edge_geometry_backward(xf, 3, edges, 2, 2, node_ptr, nullptr, 1, 1, rf, df, gxf, 3, nullptr),
           BAD, "null tensor");
    expect("backward ldx < 3", tfep_edge_geometry_backward(xf, 0, edges, 2, 2, node_ptr, incident, 0, 0, nullptr, nullptr, gxf, 3,
                                                          nullptr), BAD, "row stride");

    // pruning
    expect("workspace E < 0", tfep_edge_prune_workspace_int64s(-1), BAD, "bad size");
    expect("workspace E = 0", tfep_edge_prune_workspace_int64s(0), 1);
    expect("workspace E = 256", tfep_edge_prune_workspace_int64s(256), 2);
    expect("workspace E = 257", tfep_edge_prune_workspace_int64s(257), 3);
    expect("count E < 0", tfep_edge_prune_count(rf, -1, 1.f, ws, nullptr), BAD, "negative size");
    expect("count workspace NULL", tfep_edge_prune_count_f64(rd, 2, 1.0, nullptr, nullptr), BAD, "workspace");
    expect("count distances NULL", tfep_edge_prune_count(nullptr, 2, 1.f, ws, nullptr), BAD, "null tensor");
    expect("compact E < 0", tfep_edge_prune_compact(rf, -1, 1.f, ws, keep, 0, nullptr), BAD, "negative size");
    expect("compact n_kept < 0", tfep_edge_prune_compact_f64(rd, 2, 1.0, ws, keep, -1, nullptr), BAD, "n_kept");
    expect("compact n_kept > E", tfep_edge_prune_compact(rf, 2, 1.f, ws, keep, 3, nullptr), BAD, "n_kept");
    expect("compact E = 0", tfep_edge_prune_compact(nullptr, 0, 1.f, nullptr, nullptr, 0, nullptr), TFEP_OK);
    expect("compact none kept", tfep_edge_prune_compact_f64(rd, 2, 1.0, ws, nullptr, 0, nullptr), TFEP_OK);
    expect("compact distances NULL", tfep_edge_prune_compact(nullptr, 2, 1.f, ws, keep, 1, nullptr), BAD, "null tensor");
    expect("compact workspace NULL", tfep_edge_prune_compact_f64(rd, 2, 1.0, nullptr, keep, 1, nullptr), BAD, "null tensor");
    expect("compact keep_index NULL", tfep_edge_prune_compact(rf, 2, 1.f, ws, nullptr, 1, nullptr), BAD, "null tensor");
    expect("select E < 0", tfep_edge_select_edges(edges, -1, keep, 1, out, nullptr), BAD, "negative size");
    expect("select n_kept < 0", tfep_edge_select_edges(edges, 2, keep, -1, out, nullptr), BAD, "n_kept");
    expect("select none kept", tfep_edge_select_edges(nullptr, 2, nullptr, 0, nullptr, nullptr), TFEP_OK);
    expect("select edges NULL", tfep_edge_select_edges(nullptr, 2, keep, 1, out, nullptr), BAD, "null tensor");
    expect("select keep_index NULL", tfep_edge_select_edges(edges, 2, nullptr, 1, out, nullptr), BAD, "null tensor");
    expect("select out NULL", tfep_edge_select_edges(edges, 2, keep, 1, nullptr, nullptr), BAD, "null tensor");

    // nothing was written
    const bool untouched = ws[0] == 7 && ws[1] == 7 && gxf[0] == 0.f && gxd[0] == 0.0 && keep[0] == 0;
    if (!untouched) ++failures;
    printf("edge_ops argument checks: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
