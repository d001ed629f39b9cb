"""-m gpu: conp_potential_atom_device inside the device-resident MD loop -- variant A of tests/md_loop_ref.py
with the ordered entries, as tests/test_gpu_md_loop_ordered.py runs it, once as written and once with

    ... -> conp_ghost_fold_device(d_f, 3) -> conp_potential_atom_device(reuse_kspace = 1) -> conp_ghost_fold_device(d_pot, 1)

enqueued after the force fold of every step.  (1) x, v, q and f of the two runs are byte-identical at the end: the entry disturbs
nothing it shares scratch with.  (2) At the start, at the last step and at every re-neighbouring step the potential equals
conp_compute_potential_atom of a fresh host handle at the downloaded arrays and the conp_pair_get_list list, within 1e-11 max|pot|
(the bound of tests/test_gpu_ewald_potential.py) on the selected owned rows."""
import functools

import numpy as np
import pytest

import md_loop_ref as ml
import potential_ref as pr
from conp_amd import FixConp, capi, neighbor
from test_gpu_md_loop_ordered import Ordered, ordered_run

pytestmark = pytest.mark.gpu
VARIANT = "A"
TOL_FULL = 1e-11


def selection(c):
    """the electrode atoms and every seventh atom; eta_check: the electrode molecules"""
    s = c.s
    sel = ((s.echeck != 0) | (np.arange(c.n) % 7 == 0)).astype(np.int32)
    return sel, (s.echeck != 0).astype(np.int32)


class WithPotential(Ordered):
    """the ordered proxy; behind every fold of the forces the potential entry with reuse and its own fold.  The flags' ghost rows are
    refreshed behind every re-neighbouring (conp_ghost_fill_int_device), as for tag.  Records are taken at the start, at every
    re-neighbouring step and at the last step: a synchronisation there, nowhere else."""

    def __init__(self, fx, c, steps):
        super().__init__(fx)
        self.c, self.steps, self.loop = c, steps, None
        self.sel, self.etasel = selection(c)
        self.flags, self.targets, self.nt = capi.potential_selection(self.sel, self.etasel, c.n)
        self.records, self.rebuilt, self.calls = [], False, 0

    def post_neighbor_device(self, *a, **k):
        import torch
        super().post_neighbor_device(*a, **k)
        nall = self.loop.nall
        self.d_flags = torch.full((nall,), -1, dtype=torch.int32, device="cuda")
        self.d_flags[:self.c.n] = torch.from_numpy(self.flags).cuda()
        self.d_targets = torch.from_numpy(self.targets).cuda()
        self._fx.ghost_fill_int_device(self.d_flags.data_ptr(), 1)
        self.d_pot = torch.full((nall,), float("nan"), dtype=torch.float64, device="cuda")
        self.rebuilt = True

    def ghost_fold_device(self, d_v, width):
        self._fx.ghost_fold_device(d_v, width)
        L = self.loop
        if width != 3 or d_v != L.d_f.data_ptr():
            return
        self._fx.potential_atom_device(L.d_x.data_ptr(), L.d_q.data_ptr(), self.d_flags.data_ptr(), self.nt, self.d_targets.data_ptr(),
                                       self.d_pot.data_ptr(), eta=self.c.s.eta, reuse_kspace=True)
        self._fx.ghost_fold_device(self.d_pot.data_ptr(), 1)
        self.calls += 1
        if self.rebuilt or L.step_no == self.steps - 1:
            import torch
            torch.cuda.synchronize()
            lst, nall = self._fx.pair_get_list()
            _, ng, owner, _ = self._fx.ghost_get()
            self.records.append(dict(step=L.step_no, x=L.d_x.cpu().numpy().copy(), q=L.d_q.cpu().numpy().copy(), lst=lst, nall=nall,
                                     owner=owner.copy(), pot=self.d_pot.cpu().numpy().copy(), rebuilt=self.rebuilt))
        self.rebuilt = False


@functools.lru_cache(maxsize=None)
def potential_run():
    fx = ml.new_handle(VARIANT)
    fx.fix_transpose_list_device()
    c = ml.system(VARIANT)
    proxy = WithPotential(fx, c, ml.STEPS)
    L = ml.Loop(proxy, VARIANT, ml.STEPS, False)
    proxy.loop = L
    L.start()
    for k in range(ml.STEPS):
        L.step(k)
    res = L.result()
    fx.close()
    return res, proxy


def test_the_entry_disturbs_nothing():
    plain = ordered_run(VARIANT, 0)
    res, proxy = potential_run()
    assert proxy.calls == ml.STEPS + 1
    assert ml.same_bytes(plain, res) == [], (ml.same_bytes(plain, res), ml.first_difference(plain, res))
    assert all(v is None for v in ml.first_difference(plain, res).values())
    assert plain.builds == res.builds and sum(res.flags) >= 2


def test_the_potential_is_the_host_entry_s():
    res, proxy = potential_run()
    c = ml.system(VARIANT)
    s, n = c.s, c.n
    steps = [r["step"] for r in proxy.records]
    assert steps[0] == -1 and steps[-1] == ml.STEPS - 1
    assert [r["step"] for r in proxy.records if r["rebuilt"]] == res.builds and len(res.builds) >= 3
    own = np.nonzero(proxy.sel)[0]
    for r in proxy.records:
        nall = r["nall"]
        full = np.concatenate([np.arange(n), r["owner"]]).astype(np.int64)
        at = neighbor.Atoms(nlocal=n, nghost=nall - n, x=np.ascontiguousarray(r["x"][:nall]), q=np.ascontiguousarray(r["q"][:nall]),
                            type=s.type[full].copy(), tag=s.tag[full].copy(), echeck=s.echeck[full].copy(), owner=full.astype(np.int32))
        fh = FixConp(s, style=c.V["style"])
        fh.init_lists(r["lst"], r["lst"])
        fh.setup_post_neighbor(at)
        want = fh.compute_potential_atom(at, r["lst"], proxy.sel[full], proxy.etasel[full], eta=s.eta)
        fh.close()
        want = pr.fold(want[:nall], full, n)                         # newton on: the ghost rows onto their owners
        got = r["pot"][:n]
        e, scale = np.abs(got[own] - want[own]).max(), np.abs(want[own]).max()
        print(f"step {r['step']}: |device - host| {e:.3e}, max|pot| {scale:.3e} V")
        assert scale > 0 and e <= TOL_FULL * scale, (r["step"], e, scale)
        assert np.all(got[proxy.sel == 0] == 0.0)
