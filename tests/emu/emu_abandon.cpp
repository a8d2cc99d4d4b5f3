// TEST SCAFFOLDING -- not part of the product.  The emulator of emu_solver.cpp with two additions for the trial-abandonment tests:
// the switch (OptParams::no_trial_abandon, uph_ctx_set_trial_abandon on the device) and the line-search counters of the last run's TrajState.
#include "../../uneven_planner_amd/csrc/uph_common.hpp"
static uph::TrajState g_probe_state;
#define UPH_STATE_PROBE(st) (g_probe_state = (st))
#include "emu_solver.cpp"

extern "C" {
void emu_set_trial_abandon(void* h, int on) { ((Emu*)h)->P.no_trial_abandon = on ? 0 : 1; }
// out[5]: rejected, guarded, abandoned before the samples, chunks skipped, adjoints skipped
// the product's rule (Solver::noExitAfterRejection) for a trial that is the (count + 1)-th of its search
int emu_may_abandon(int count, double stp, double mu, double stpmin, double stpmax, int max_linesearch, double machine_prec) {
    return Solver<HostWG>::noExitAfterRejection(count, stp, mu, stpmin, stpmax, max_linesearch, machine_prec) ? 1 : 0;
}
void emu_abandon_counters(long long* out) {
    out[0] = g_probe_state.ls_rejected; out[1] = g_probe_state.ls_guarded; out[2] = g_probe_state.ls_abandoned;
    out[3] = g_probe_state.chunks_skipped; out[4] = g_probe_state.adjoints_skipped;
}
}
