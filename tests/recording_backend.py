"""TEST-ONLY backend: a fake with the full capability set of HipBackend that runs on CPU tensors,
does no arithmetic and records every call the MPC class makes (tests/test_mpc_launch_trace.py).
It is never importable from the product package.

One record per call, a flat list that starts with the method name:

  solve_lin     al_iter, max_newton, flags, n_ls, variant, workspace, factor?, info?, skip?, newton_counts?
  solve_nonlin  al_iter, max_newton, flags, workspace, info?, skip?, newton_counts?
  exit_test     mode
  newton_step   workspace, factor?, info?, obs kind
  merit         K, obs kind
  merit_pick    n_ls, obs kind
  dual_update   obs kind
  backward      factor, F
  backward_ws   workspace, F

flags are spelled ("INIT_MERIT|DUAL_UPDATE"), a workspace is None, "cached" or "private<k>" (the k-th one handed out
by new_workspace / new_workspace_nonlin), `x?` says whether the argument was passed, an obs kind is None,
"state_estimator" or "obstacles", a factor is "factor<k>" (the k-th distinct packed-factor tensor a launch was given)
and F is "caller" (the tensor note_caller_F named), "nonlin_F_view", "last_linearisation" (the F of the last
newton_step) or "linearisation<k>".

The five behaviours the host logic needs to take its real branches:
  * solve_lin / solve_nonlin with newton_counts return False (nothing done) when built with coop_ok=False;
  * a launch with ALQP_DUAL_UPDATE, or dual_update, multiplies rho by rho_scale;
  * last_variant follows HipBackend's rule: team when ALQP_SAVE_FACTOR is set or B < QUAD_MIN_BATCH, else quad,
    unless a variant is given; like HipBackend, solve_lin sets it before the launch, a refused one included;
  * barrier_timeout=True writes -1 into newton_counts, bad_info=True sets info[0] non-zero;
  * merit and every solve launch that ran fill rnorm2 with a value half the one before, so the frozen-linearisation
    stream loop (which goes on while the mean residual falls) runs until rho passes rho_max.
So that counts read back from the device differ from MAX_NEWTON, a cooperative launch reports COUNTED Newton steps
per AL iteration and exit_test raises its exit flag after COUNTED steps."""
import torch

FLAG_NAMES = ((1, "INIT_MERIT"), (2, "DUAL_UPDATE"), (4, "SAVE_FACTOR"), (8, "WS_PRIMED"), (16, "EXIT_IN_KERNEL"))
SAVE_FACTOR, DUAL_UPDATE = 4, 2
COUNTED = 3


def flag_str(flags):
    names = [n for bit, n in FLAG_NAMES if flags & bit]
    rest = flags & ~sum(bit for bit, _ in FLAG_NAMES)
    return "|".join(names + ([str(rest)] if rest else [])) or "0"


def _obs_kind(obs):
    if obs is None:
        return None
    return obs if isinstance(obs, str) else "obstacles"


class RecordingBackend:
    name = "recording-test"
    supports_exit_in_kernel = True
    QUAD_MIN_BATCH = 4

    def __init__(self, coop_ok=True, barrier_timeout=False, bad_info=False):
        self.coop_ok, self.barrier_timeout, self.bad_info = coop_ok, barrier_timeout, bad_info
        self.calls = []
        self._cached = None
        self._private = []
        self._factors = []
        self._F_views = []
        self._lins = []
        self._caller_F = None
        self._rn2 = 1.0

    # -- naming of the objects a call was given ---------------------------------------
    def note_caller_F(self, F):
        self._caller_F = F

    def _ws_name(self, ws):
        if ws is None:
            return None
        if self._cached is not None and ws.data_ptr() == self._cached.data_ptr():
            return "cached"
        for k, w in enumerate(self._private):
            if w.data_ptr() == ws.data_ptr():
                return f"private{k}"
        return "unknown"

    def _note_factor(self, factor):
        if factor is not None and not any(f.data_ptr() == factor.data_ptr() for f in self._factors):
            self._factors.append(factor)

    def _factor_name(self, factor):
        for k, f in enumerate(self._factors):
            if f.data_ptr() == factor.data_ptr():
                return f"factor{k}"
        return "unknown"

    def _F_name(self, F):
        same = lambda t: t is not None and t.data_ptr() == F.data_ptr() and t.shape == F.shape
        if same(self._caller_F):
            return "caller"
        if any(same(v) for v in self._F_views):
            return "nonlin_F_view"
        if self._lins and same(self._lins[-1]):
            return "last_linearisation"
        for k, v in enumerate(self._lins):
            if same(v):
                return f"linearisation{k}"
        return "unknown"

    # -- capabilities ---------------------------------------------------------------------
    def supported(self, B, T, nx, nu, dtype):
        return True

    def qps_per_wave(self, B, T, nx, nu, dtype):
        return 1

    def _workspace(self, dims, like):
        if self._cached is None:
            self._cached = torch.zeros(4, dtype=like.dtype)
        return self._cached, 4 * like.element_size()

    def new_workspace(self, dims, like):
        self._private.append(torch.zeros(4, dtype=like.dtype))
        return self._private[-1]

    new_workspace_nonlin = new_workspace

    def nonlin_F_view(self, ws, dims):
        B, T, nx, nu = dims
        self._F_views.append(torch.zeros(B, T - 1, nx, nx + nu, dtype=ws.dtype))
        return self._F_views[-1]

    # -- launches ---------------------------------------------------------------------------
    def _residual(self, rnorm2):
        if rnorm2 is not None:
            self._rn2 *= 0.5
            rnorm2.fill_(self._rn2)

    def _launch(self, flags, rho, rho_scale, info, newton_counts, rnorm2):
        """What every solve launch does to its outputs. False: a refused cooperative launch."""
        if newton_counts is not None:
            if not self.coop_ok:
                return False
            newton_counts.fill_(-1 if self.barrier_timeout else COUNTED)
        self._residual(rnorm2)
        if flags & DUAL_UPDATE:
            rho.mul_(rho_scale)
        if self.bad_info and info is not None:
            info[0] = 1
        return True

    def solve_lin(self, dims, Qd, q, F, c, x0, ulo, uhi, sb_u, st_u, z, lam, rho, phi, rnorm2=None, info=None,
                  status=None, factor=None, al_iter=2, max_newton=4, n_ls=20, flags=3, rho_scale=10.0, trace=None,
                  variant=None, workspace=None, skip=None, newton_counts=None, exit_tol=1e-3):
        self._note_factor(factor)
        self.calls.append(["solve_lin", al_iter, max_newton, flag_str(flags), n_ls, variant, self._ws_name(workspace),
                           factor is not None, info is not None, skip is not None, newton_counts is not None])
        if variant in (None, "auto"):
            variant = "team" if (flags & SAVE_FACTOR) or dims[0] < self.QUAD_MIN_BATCH else "quad"
        self.last_variant = variant
        return self._launch(flags, rho, rho_scale, info, newton_counts, rnorm2)

    def solve_nonlin(self, dims, dyn_id, dyn_h, Qd, q, x0, ulo, uhi, sb_u, st_u, z, lam, rho, phi, rnorm2=None,
                     info=None, status=None, al_iter=2, max_newton=4, flags=3, rho_scale=10.0, skip=None,
                     workspace=None, newton_counts=None, exit_tol=1e-3):
        self.calls.append(["solve_nonlin", al_iter, max_newton, flag_str(flags), self._ws_name(workspace),
                           info is not None, skip is not None, newton_counts is not None])
        if not self._launch(flags, rho, rho_scale, info, newton_counts, rnorm2):
            return False
        self.last_variant = "quad"
        return True

    def exit_test(self, sumsq, ctl, mode, tol=1e-3):
        self.calls.append(["exit_test", mode])
        if mode == 0:
            ctl.zero_()
        elif float(ctl[0]) == 0.0:
            ctl[1] += 1.0
            if float(ctl[1]) >= COUNTED:
                ctl[0] = 1.0

    def newton_step(self, dims, z, xnext, F, x0, lam, rho, Qd, q, ulo, uhi, sb_u, st_u, d_out, g_out=None,
                    factor=None, info=None, obs=None, workspace=None):
        self._note_factor(factor)
        self._lins.append(F)
        self.calls.append(["newton_step", self._ws_name(workspace), factor is not None, info is not None,
                           _obs_kind(obs)])
        d_out.zero_()
        if self.bad_info and info is not None:
            info[0] = 1

    def merit(self, dims, K, zc, xnext, x0, lam, rho, Qd, q, ulo, uhi, sb_u, st_u, phi, rnorm2=None, obs=None):
        self.calls.append(["merit", K, _obs_kind(obs)])
        self._residual(rnorm2)

    def merit_pick(self, dims, n_ls, d, xnext_all, x0, lam, rho, Qd, q, ulo, uhi, sb_u, st_u, z, phi_prev,
                   rnorm2=None, phi_all=None, k_out=None, accept_out=None, obs=None):
        self.calls.append(["merit_pick", n_ls, _obs_kind(obs)])

    def dual_update(self, dims, z, xnext, x0, ulo, uhi, sb_u, st_u, lam, rho, rho_scale=10.0, obs=None):
        self.calls.append(["dual_update", _obs_kind(obs)])
        rho.mul_(rho_scale)

    def backward(self, dims, factor, F, rho, z_final, gbar, q_grad, Qd_grad):
        self.calls.append(["backward", self._factor_name(factor), self._F_name(F)])
        q_grad.zero_()
        Qd_grad.zero_()

    def backward_ws(self, dims, workspace, F, rho, z_final, gbar, q_grad, Qd_grad):
        self.calls.append(["backward_ws", self._ws_name(workspace), self._F_name(F)])
        q_grad.zero_()
        Qd_grad.zero_()
