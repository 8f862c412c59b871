// switches_probe — prints a few rows of the switch table (zgml_amd/csrc/switches.h) for tests/test_switches.py. One process per
// case, so that the table's latch is fresh. Built twice: plain and with -DZGML_TRACE.
//   switches_probe                 the rows, once
//   switches_probe NAME VALUE      the rows; then setenv(NAME, VALUE), and the rows (latched) and the per-context switches again
#include <stdio.h>
#include <stdlib.h>

#include "../../zgml_amd/csrc/switches.h"

struct FakeCtx { // the fields read_ctx_switches touches, with the defaults of zgml_hip_ctx
    bool opt_graph = true, opt_fusion = true, opt_ksplit = false, opt_w8a8 = false, host_prof = false;
};

static void rows(const char* tag) {
    const zgml::Switches& s = zgml::sw();
    printf("%s qmv_xdirect=%d qmm_waves=%d hip_nt_min_bytes=%llu copy_variant=%d hip_elt_vec4_min=%u debug_plan_set=%d debug_plan=%d "
           "qmm_xdl5_trace=%d hip_debug_skip_grid=%d hip_skip_kinds=%u graph_dump=%s\n",
           tag, (int)s.qmv_xdirect, s.qmm_waves, (unsigned long long)s.hip_nt_min_bytes, s.copy_variant, s.hip_elt_vec4_min,
           (int)s.hip_debug_plan.set, s.hip_debug_plan.value, (int)s.qmm_xdl5_trace, s.hip_debug_skip_grid, s.hip_skip_kinds,
           s.hip_graph_dump ? s.hip_graph_dump : "(null)");
}
static void ctx(const char* tag) {
    FakeCtx c;
    zgml::read_ctx_switches(c);
    printf("%s graph=%d fusion=%d ksplit=%d w8a8=%d host_prof=%d\n", tag, (int)c.opt_graph, (int)c.opt_fusion, (int)c.opt_ksplit, (int)c.opt_w8a8,
           (int)c.host_prof);
}

int main(int argc, char** argv) {
    rows("first");
    ctx("ctx_first");
    if (argc == 3) {
        setenv(argv[1], argv[2], 1);
        rows("second");
        ctx("ctx_second");
    }
    return 0;
}
