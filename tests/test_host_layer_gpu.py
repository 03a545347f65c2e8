"""-m gpu: lifetimes and dispatch of the Python host layer (gym_comm_amd.vec_env / batched).  A replaced
partner closes the prepared step it was stepped with and retires the closed loops built on it; an ego
given as an ``act_into`` object or as a bare callable drives a closed loop to what ``step_tensors`` does
with the same actions.  open-divider_tomato, C = 2, 130 envs: two full groups of 64 and a partial one."""
import gc
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

N, C, T, STEPS = 130, 2, 4, 6           # T = 4: every env is auto-reset inside the 6 steps
OUTPUTS = ("state", "obs", "shaped_reward", "done", "ep_return", "ep_length", "comm", "timestep")


def _arg():
    return SimpleNamespace(level="open-divider_tomato", num_agents=2, max_num_timesteps=T, ego_config={},
                           partner_config={}, num_communication=C, communication_on=True, ego_led=False,
                           fow_radius=2)


def _tape(steps, seed=0):
    gen = torch.Generator().manual_seed(seed)
    return [torch.stack([torch.randint(0, 4, (N,), generator=gen), torch.randint(0, C, (N,), generator=gen)],
                        dim=1).to(torch.int32).cuda() for _ in range(steps)]


def _outputs(venv):
    return {name: getattr(venv._b, name).clone() for name in OUTPUTS}


class _CountingLib:
    """The batch's library with ``oc_call_destroy`` counted; everything else passes through."""

    def __init__(self, lib):
        self._lib, self.destroyed = lib, []

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def oc_call_destroy(self, handle):
        self.destroyed.append(handle.value)
        return self._lib.oc_call_destroy(handle)


def test_a_replaced_partner_closes_its_prepared_step_exactly_once():
    from gym_comm_amd.vec_env import OvercookedVecEnv, RandomPartner
    venv = OvercookedVecEnv(_arg(), N, seed=3)
    b = venv._b
    b._L = lib = _CountingLib(b._L)
    tape = _tape(8)
    venv.reset_tensors()
    venv.step_tensors(tape[0])
    assert len(b._prepared) == 1 and venv._fast["prepared"] is b._prepared[0]
    dropped = []
    for k in range(5):
        old = b._prepared[0]
        if k == 4:      # the last configuration: the state it starts from
            before = b.get_state()
        venv.partner = pt = RandomPartner(C, seed=10 + k, device=b.device)
        assert old.closed and b._prepared == [] and venv._fast is None
        dropped.append(old)
        assert len(lib.destroyed) == k + 1
        if k == 4:
            pt_before = pt.get_state(N)
        venv.step_tensors(tape[1 + k])
        assert len(b._prepared) == 1 and b._prepared[0] is not old and not b._prepared[0].closed
    # five distinct prepared steps, one destroy each (the allocator may hand a freed address out again,
    # so the handles' values need not differ)
    assert len({id(old) for old in dropped}) == len(lib.destroyed) == 5 and None not in lib.destroyed
    for old in dropped:
        old.close()                                                     # idempotent: nothing more is destroyed
        with pytest.raises(RuntimeError):
            old(None, False)
    assert len(lib.destroyed) == 5
    # the last configuration steps as a fresh env given the same partner and state does
    fresh = OvercookedVecEnv(_arg(), N, seed=99, partner=RandomPartner(C, seed=14, device=b.device))
    fresh.reset_tensors()
    fresh._b.set_state(before)
    fresh.partner.set_state(pt_before)
    fresh.step_tensors(tape[5])
    for k in (6, 7):
        for name, want in _outputs(fresh).items():
            assert torch.equal(getattr(b, name), want), (k, name)
        assert torch.equal(venv._act[2:4], fresh._act[2:4]), k           # the partner's reported draw
        venv.step_tensors(tape[k])
        fresh.step_tensors(tape[k])
    for name, want in _outputs(fresh).items():
        assert torch.equal(getattr(b, name), want), name
    live = b._prepared[0]
    del venv, fresh, b
    gc.collect()                                                         # the batch closes what is left as it goes
    assert live.closed and len(lib.destroyed) == 6


def test_closed_loops_retire_when_the_partner_is_replaced():
    from gym_comm_amd.vec_env import OvercookedVecEnv, RandomPartner
    venv = OvercookedVecEnv(_arg(), N, seed=3)
    venv.reset_tensors()
    loop = venv.closed_loop(RandomPartner(C, seed=9), graph=False)
    assert loop.partner is venv.partner and loop in venv._loops and not loop.retired
    loop.step()
    venv.partner = RandomPartner(C, seed=5)
    assert loop.retired and len(venv._loops) == 0
    state = venv._b.state.clone()
    for call in (loop.step, loop.enqueue):
        with pytest.raises(RuntimeError) as e:
            call()
        assert "partner" in str(e.value) and "new loop" in str(e.value)
    assert torch.equal(venv._b.state, state)                            # a retired loop launches nothing
    new = venv.closed_loop(RandomPartner(C, seed=9), graph=False)
    assert new.partner is venv.partner and list(venv._loops) == [new]
    obs, rew, done = new.step()
    assert not torch.equal(venv._b.state, state) and rew.shape == done.shape == (N,)
    assert venv._b.read_metrics()["env_steps"] == 2 * N


def test_reset_after_the_partner_of_a_one_launch_loop_was_replaced():
    """``reset_tensors()`` primed -- and rewound the streams of -- every loop ever built, with
    the env's CURRENT partner: an AttributeError once that was no ``FusedMLPPartner``."""
    from gym_comm_amd.vec_env import FusedMLPPartner, MLPPolicy, OvercookedVecEnv, TorchPolicyPartner
    venv = OvercookedVecEnv(_arg(), N, seed=3)
    S = venv._b.S
    ego = FusedMLPPartner(MLPPolicy(S, C, seed=1).cuda(), sample=True, seed=7)
    venv.partner = alt = FusedMLPPartner(MLPPolicy(S, C, seed=2).cuda(), sample=True, seed=8)
    venv.reset_tensors()
    if venv._b.kernel_flavour != "spec":
        pytest.skip("the fused policies are built into the specialised libraries only")
    loop = venv.closed_loop(ego, graph=False, one_launch=True)
    assert loop.one_launch and loop.partner is alt
    loop.step()
    streams = ego._rng.clone(), alt._rng.clone()
    venv.partner = TorchPolicyPartner(MLPPolicy(S, C, seed=4).cuda(), sample=False)
    venv.reset_tensors()                                                # returns
    assert loop.retired and len(venv._loops) == 0
    assert torch.equal(ego._rng, streams[0]) and torch.equal(alt._rng, streams[1])     # nobody rewound them
    with pytest.raises(RuntimeError) as e:
        loop.step()
    assert "partner" in str(e.value)
    new = venv.closed_loop(ego, graph=False)
    assert not new.one_launch and new.partner is venv.partner
    new.step()
    assert venv._b.read_metrics()["env_steps"] == 2 * N


@pytest.fixture(scope="module")
def stepped_by_tensors():
    """The tape of 6 ego actions through ``step_tensors``: every output after every step."""
    from gym_comm_amd.vec_env import OvercookedVecEnv
    venv = OvercookedVecEnv(_arg(), N, seed=3)
    venv.reset_tensors()
    tape, out = _tape(STEPS, seed=1), []
    for a in tape:
        venv.step_tensors(a)
        out.append(_outputs(venv))
    assert int(sum(o["done"].sum() for o in out)) == N                  # the auto-reset was part of it
    return tape, out


class _ActInto:
    """A player with nothing but ``act_into``."""

    def __init__(self, tape):
        self.tape = iter(tape)

    def act_into(self, obs, move_row, comm_row):
        a = next(self.tape)
        move_row.copy_(a[:, 0])
        comm_row.copy_(a[:, 1])


def _callable(tape, dtype):
    it = iter(tape)
    return lambda obs: next(it).to(dtype)


@pytest.mark.parametrize("form", ["act_into", "callable-int32", "callable-int64"])
def test_an_ego_of_every_form_drives_the_loop_as_step_tensors_does(form, stepped_by_tensors):
    """``seat_actions`` on the ego seat: an object with only ``act_into`` writes the ego's rows; a bare
    callable's int32 [n][2] is consumed as it lies; its int64 result goes through the rows."""
    from gym_comm_amd.vec_env import OvercookedVecEnv
    tape, want = stepped_by_tensors
    ego = {"act_into": lambda: _ActInto(tape), "callable-int32": lambda: _callable(tape, torch.int32),
           "callable-int64": lambda: _callable(tape, torch.int64)}[form]()
    assert hasattr(ego, "act_into") == (form == "act_into")
    venv = OvercookedVecEnv(_arg(), N, seed=3)
    first = venv.reset_tensors()
    loop = venv.closed_loop(ego, graph=False)
    for k in range(STEPS):
        obs, rew, done = loop.step()
        assert obs is first and rew is venv._b.shaped_reward and done is venv._b.done
        for name, t in want[k].items():
            assert torch.equal(getattr(venv._b, name), t), (form, k, name)
        assert torch.equal(obs.rows, want[k]["obs"][0]), (form, k)
