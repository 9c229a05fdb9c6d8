// extern "C" view of pnpflow_amd/csrc/rk45_control.h for tests/test_prior_eval_host.py (host clang++ only, loaded with ctypes).
#include "rk45_control.h"

extern "C" {
// tables: out[6] C, out[30] A (row-major [6][5]), out[6] B, out[7] E
void rk_tables(double* c, double* a, double* b, double* e) {
    for (int i = 0; i < 6; ++i) { c[i] = rk45::C[i]; b[i] = rk45::B[i]; for (int j = 0; j < 5; ++j) a[i * 5 + j] = rk45::A[i][j]; }
    for (int i = 0; i < 7; ++i) e[i] = rk45::E[i];
}
double rk_initial_probe_step(double d0, double d1, double interval) { return rk45::initial_probe_step(d0, d1, interval); }
double rk_initial_step(double h0, double d1, double d2, double interval) { return rk45::initial_step(h0, d1, d2, interval); }

rk45::Controller* rk_new(double t0, double t_bound, double h_abs, long long max_attempts) { return new rk45::Controller(t0, t_bound, h_abs, max_attempts); }
void rk_delete(rk45::Controller* c) { delete c; }
// -> status; h_tnew[2] = (h, t_new) of the opened attempt
int rk_begin(rk45::Controller* c, double* h_tnew) { const int s = c->begin(); h_tnew[0] = c->h; h_tnew[1] = c->t_new; return s; }
// -> status; *accepted = 1 when the state advances
int rk_end(rk45::Controller* c, double error_norm, int* accepted) { bool a = false; const int s = c->end(error_norm, &a); *accepted = a ? 1 : 0; return s; }
// out[4] = (t, h_abs, accepted, rejected)
void rk_state(const rk45::Controller* c, double* out) { out[0] = c->t; out[1] = c->h_abs; out[2] = (double)c->accepted; out[3] = (double)c->rejected; }
}
