"""Deep ensembles of the voltage network: E equal networks trained and evaluated in the launches of one.

MC-dropout (`get_MC_samples`) is one source of the epistemic column of the results array; the standard alternative is a deep
ensemble -- E copies of `DNN(p, logvar, layers)` with E initialisations, trained on the same rows and read as a mixture.  At the
reference's sizes (1e3 .. 1e4 rows) a training step of one network is a chain of short dependent launches that leaves the chip
idle, so E networks trained one after another cost E times that chain; here every kernel of the any-width family
(csrc/pinn_general.hip) takes the member from its launch grid (`pinn_gens_*`), and a step of the ensemble is as many launches
as a step of one network.

The batched calls are exact: member m of `pinn_gens_forward` / `_train_grads` / `_train_step` is bit for bit the `pinn_gnet_*` call
on member m's parameters with dropout seed `seed + m`.  `DeepEnsemble(layers, E, p, seed=s)` therefore IS the E models
`DNN(p, logvar, layers, seed=s + m, kernels="general")` built one after another (same torch initial values, same Philox streams),
and `fit` IS `train_dnn` of each of them: same schedule, same stream positions, same bytes (tests/test_gpu_ensemble.py).

    ens = DeepEnsemble([8, 64, 64, 1], n_members=8, p=0.2)
    ens.fit(x, y, 12002)
    pred_mean, a_u, e_u = ens.predict(X)                      # the tuple get_MC_samples returns
    arr = create_comprehensive_results_array_v2(model, dataset, ensemble=ens)      # columns 9-11 from the ensemble

Combine (`pinn_gens_combine`, one thread per row, sums in double): pred_mean = mean_m u_m; e_u = sqrt(mean_m u_m^2 - pred_mean^2)
(population form, as get_MC_samples); a_u = sqrt(exp(mean_m logvar_m)) for rule "mc" (get_MC_samples' form: column 10 keeps its
meaning) or sqrt(mean_m exp(logvar_m)) for rule "mixture" (the mixture variance of the deep-ensembles literature).

Out of scope: members trained on different rows (bagging, folds, per-stack models); members of different layers lists;
MC-dropout inside each member (predict runs the members in eval mode); autograd through the batched calls (use `member(m)`);
data parallelism; the fused and wide kernel families (an ensemble runs on the any-width kernels, exact fp32, whatever its widths).
"""
import ctypes

import numpy as np
import torch

from . import _lib, layout

RULES = {"mc": 0, "mixture": 1}
STATE_VERSION = 1
MAX_MEMBERS = 32


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class DeepEnsemble:
    """E networks DNN(p, logvar, layers) on one device buffer [E, P] (P = pinn_gnet_param_count, state_dict layout per member)."""

    def __init__(self, layers, n_members, p, logvar=True, seed=0):
        """Member m is initialised as `DNN(p, logvar, layers, seed=seed + m, kernels="general")` initialises, the members built in
        index order (torch's global generator gives the initial values, as for any DNN), and draws that model's dropout masks."""
        from .model import DNN
        self._setup(layers, n_members, p, logvar, seed)
        for m in range(self.n_members):
            self._flat[m].copy_(DNN(p, logvar, self.layers, seed=self.seed + m, kernels="general").flat_params())

    def _setup(self, layers, n_members, p, logvar, seed):
        from .model import _device
        dev = _device()                      # raises without a GPU, like DNN
        self._lib = _lib.load()
        self.layers = [int(v) for v in layers]
        layout.check_general(self.layers)
        self.n_members = int(n_members)
        if not 1 <= self.n_members <= MAX_MEMBERS:
            raise ValueError("n_members must be in 1 .. %d (got %r)" % (MAX_MEMBERS, n_members))
        self.p, self.logvar, self.seed = float(p), bool(logvar), int(seed)
        self._gnet = _lib.GNet(self.layers)
        self.n_params = int(self._lib.pinn_gnet_param_count(ctypes.byref(self._gnet)))
        if self.n_params <= 0:
            raise _lib.PinnError("pinn_gnet_param_count rejected layers %r" % (self.layers,))
        shape = (self.n_members, self.n_params)
        self._flat = torch.zeros(shape, dtype=torch.float32, device=dev)
        self._grad = torch.zeros(shape, dtype=torch.float32, device=dev)
        self._adam_m = torch.zeros(shape, dtype=torch.float32, device=dev)
        self._adam_v = torch.zeros(shape, dtype=torch.float32, device=dev)
        self._work = None
        self._step_counter = 0               # position in the dropout stream: one per training step, across fit calls (as train_dnn)
        self.losses = np.zeros((0, self.n_members))
        self.loss_epochs = []
        self.last_loss = None
        self.verbose = True

    @classmethod
    def from_models(cls, models):
        """An ensemble of trained models (DNN(kernels="general") or PhysicsInformedNN around one) of equal layers; parameters are
        copied.  p, logvar and the base seed are those of models[0]: member m continues with dropout seed models[0].seed + m."""
        dnns = [getattr(m, "dnn", m) for m in models]
        if not dnns:
            raise ValueError("from_models needs at least one model")
        first = dnns[0]
        for d in dnns:
            if d.layer_sizes != first.layer_sizes:
                raise ValueError("members must share one layers list (%s against %s)" % (d.layer_sizes, first.layer_sizes))
        ens = cls.__new__(cls)
        ens._setup(first.layer_sizes, len(dnns), first.p, first.logvar, first.seed)
        for m, d in enumerate(dnns):
            ens._flat[m].copy_(d.flat_params())
        return ens

    # ------------------------------------------------------------------ plumbing
    def _rows(self, X):
        X = torch.as_tensor(X).detach().to(self._flat.device, torch.float32)
        return X.reshape(-1, self.layers[0]).contiguous()

    def _workspace(self, n_rows):
        nb = self._lib.pinn_gens_workspace_bytes(ctypes.byref(self._gnet), self.n_members, int(n_rows))
        if nb == 0:
            raise _lib.PinnError("pinn_gens_workspace_bytes rejected the network")
        if self._work is None or self._work.numel() < nb:
            self._work = None                # free the smaller one first
            self._work = torch.empty(nb, dtype=torch.uint8, device=self._flat.device)
        return self._work

    def dropout_struct(self, stream_id, row_offset=0):
        """The struct of a batched training call: DNN.dropout_struct of member 0; the kernels add the member to the seed."""
        d = _lib.Dropout()
        d.mode = _lib.DROP_PHILOX
        for l in range(len(self.layers) - 1):          # k hidden layers + the variance head's first layer
            d.p[l] = self.p
        d.seed = self.seed & 0xFFFFFFFFFFFFFFFF
        d.stream = int(stream_id) & 0xFFFFFFFF
        d.row_offset = int(row_offset)
        d.d_bits = None
        d.d_step_counter = None
        return d

    # ------------------------------------------------------------------ training
    def train_step(self, x, y, lr, step):
        """One full-batch step of every member (device tensors x [N, 8], y [N]): gradients + Adam.  Returns the members' raw loss
        sums, float64 [E, 4] on the device (nll, |logvar|, (y - u)^2, sum dL/du).  Advances the dropout stream by one."""
        n = x.shape[0]
        work = self._workspace(n)
        self._step_counter += 1
        drop = self.dropout_struct(self._step_counter) if self.p > 0 else None
        loss = torch.empty(self.n_members, 4, dtype=torch.float64, device=x.device)
        rc = self._lib.pinn_gens_train_step(ctypes.byref(self._gnet), self.n_members, _ptr(self._flat), _ptr(x), _ptr(y), n, max(1, n),
                                            ctypes.byref(drop) if drop is not None else None, _ptr(self._grad), _ptr(loss), _ptr(work),
                                            work.numel(), _ptr(self._adam_m), _ptr(self._adam_v), lr, step, _stream())
        _lib.check(rc, "pinn_gens_train_step")
        return loss

    def fit(self, x, y, nIter):
        """train_dnn (01:929-964) for all members at once: full-batch Adam(lr=0.01) + StepLR(1000, 0.8), a fresh optimizer per call,
        one dropout-stream position per step; a line every 1000 steps (one host read each, none per step).  `losses` gets one row
        [E] per line and one for the last step, `loss_epochs` their epochs."""
        x = self._rows(x)
        y = torch.as_tensor(y).detach().to(x.device, torch.float32).reshape(-1).contiguous()
        n = x.shape[0]
        if y.numel() != n:
            raise ValueError("x has %d rows, y %d" % (n, y.numel()))
        self._adam_m.zero_(); self._adam_v.zero_()
        self._log('============ deep ensemble training (%d members) ============' % self.n_members)
        self._log('  Epoch |  mean Loss |  min Loss  |  max Loss  |    LR    ')
        hist, epochs = [], []

        def per_member(sums):
            ls = sums.cpu().numpy()           # fp64 [E, 4]: the one host read of a log line
            return (ls[:, 0] + 0.01 * ls[:, 1]) / max(1, n)
        sums = None
        for epoch in range(int(nIter)):
            if n == 0:
                break
            sums = self.train_step(x, y, 0.01 * 0.8 ** (epoch // 1000), epoch + 1)
            if epoch % 1000 == 0:
                lo = per_member(sums)
                hist.append(lo); epochs.append(epoch)
                self._log(f' {epoch:5d}  | {lo.mean():10.3e} | {lo.min():10.3e} | {lo.max():10.3e} | {0.01 * 0.8 ** ((epoch + 1) // 1000):8.1e}')
        if sums is not None:
            lo = per_member(sums)
            hist.append(lo); epochs.append(int(nIter) - 1)
            self.last_loss = lo
            self._log(f'ensemble training done, final loss: mean {lo.mean():.3e}, worst member {lo.max():.3e}')
        if hist:
            self.losses = np.concatenate([self.losses, np.stack(hist)], axis=0)
            self.loss_epochs += epochs
        return self

    def _log(self, *a):
        if self.verbose:
            print(*a)

    # ------------------------------------------------------------------ inference
    def forward(self, x):
        """(u [E, N], logvar [E, N]) device tensors: every member's eval forward (dropout off) in one call.  logvar=False: zeros."""
        x = self._rows(x)
        n = x.shape[0]
        u = torch.empty(self.n_members, n, dtype=torch.float32, device=x.device)
        lv = torch.empty(self.n_members, n, dtype=torch.float32, device=x.device)
        work = self._workspace(n)
        rc = self._lib.pinn_gens_forward(ctypes.byref(self._gnet), self.n_members, _ptr(self._flat), _ptr(x), n, None, _ptr(u), _ptr(lv),
                                         _ptr(work), work.numel(), _stream())
        _lib.check(rc, "pinn_gens_forward")
        if not self.logvar:
            lv = torch.zeros_like(u)
        return u, lv

    def combine(self, u, logvar, rule="mc"):
        """(pred_mean, a_u, e_u) device tensors [N] of per-member u, logvar [E, N] (pinn_gens_combine; see the module docstring)."""
        if rule not in RULES:
            raise ValueError("rule must be 'mc' or 'mixture' (got %r)" % (rule,))
        u, logvar = u.contiguous(), logvar.contiguous()
        e, n = u.shape
        out = torch.empty(3, n, dtype=torch.float32, device=u.device)
        rc = self._lib.pinn_gens_combine(_ptr(u), _ptr(logvar), e, n, RULES[rule], _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _stream())
        _lib.check(rc, "pinn_gens_combine")
        return out[0], out[1], out[2]

    def predict(self, X, rule="mc", device_output=False):
        """(pred_mean [N], a_u [N], e_u [N]) float32 numpy in normalised units -- the tuple get_MC_samples returns, with the members
        in place of the stochastic passes.  device_output=True keeps the three tensors on the device."""
        out = self.combine(*self.forward(X), rule=rule)
        return out if device_output else tuple(o.cpu().numpy() for o in out)

    # ------------------------------------------------------------------ members and state
    def member(self, m):
        """A DNN(kernels="general") holding a copy of member m's parameters, with member m's dropout seed.  (The torch initial
        values the constructor draws are overwritten; the global generator is left where it was.)"""
        from .model import DNN
        m = range(self.n_members)[m]
        with torch.random.fork_rng(devices=[]):
            dnn = DNN(self.p, self.logvar, self.layers, seed=self.seed + m, kernels="general")
        dnn.flat_params().copy_(self._flat[m])
        return dnn

    def state_dict(self):
        """Tensors only (loads with torch.load(..., weights_only=True), like save_checkpoint's file)."""
        return {"version": torch.tensor(STATE_VERSION), "layers": torch.tensor(self.layers), "n_members": torch.tensor(self.n_members),
                "params": self._flat.detach().cpu().clone(), "adam.m": self._adam_m.detach().cpu().clone(),
                "adam.v": self._adam_v.detach().cpu().clone(), "p": torch.tensor(self.p, dtype=torch.float64),
                "logvar": torch.tensor(self.logvar), "counters": torch.tensor([self._step_counter, self.seed], dtype=torch.int64)}

    def load_state_dict(self, sd):
        """Restores what state_dict wrote into an ensemble of the same layers and size; ValueError on a mismatch."""
        if int(sd["version"]) != STATE_VERSION:
            raise ValueError("ensemble state version %d, expected %d" % (int(sd["version"]), STATE_VERSION))
        if sd["layers"].tolist() != self.layers or int(sd["n_members"]) != self.n_members:
            raise ValueError("state is for %d members of layers %s, the ensemble has %d of %s"
                             % (int(sd["n_members"]), sd["layers"].tolist(), self.n_members, self.layers))
        self._flat.copy_(sd["params"])
        self._adam_m.copy_(sd["adam.m"])
        self._adam_v.copy_(sd["adam.v"])
        self.p, self.logvar = float(sd["p"]), bool(sd["logvar"])
        c = sd["counters"].tolist()
        self._step_counter, self.seed = int(c[0]), int(c[1])
        return self
