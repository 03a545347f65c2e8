"""-m gpu: host-mapped I/O of the numpy boundary (include/oc_hostio.h, ``OvercookedVecEnv(host_io="mapped")``).

``oc_pack_host_tiled`` writes the bytes ``oc_pack_host`` writes -- into device memory and into an
``oc_hostio_alloc`` buffer read on the host -- and nothing behind them; a mapped env returns what a
copying env returns, step by step, on the single-launch path and on the slow one; ``step_async`` /
``step_wait`` keep their protocol; the mapped memory lives as long as an array of it does."""
import gc
import weakref
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CANARY, FILL = 64, 0xA5
I32 = np.iinfo(np.int32)


def _lib_hostio():
    from gym_comm_amd import _lib
    return _lib, _lib.load(lib="hostio")


def _salad_widths():
    """The plan ``hostio.pack_plan`` makes for open-divider_salad with 3 comm channels, restated."""
    from gym_comm_amd import compiler
    from gym_comm_amd.batched import obs_layout
    from gym_comm_amd.vec_env import SPACE_DTYPE
    S, C = compiler.compile_level("open-divider_salad", 2, 30).num_subtasks, 3
    F = 22 + S + 2 * C
    block_of = {np.dtype(np.int64): 0, np.dtype(np.float32): 1, np.dtype(np.int8): 2}
    width, plan = [0, 0, 0], np.zeros(F, np.int32)
    for k, (lo, hi) in obs_layout(S, C).items():
        blk = block_of[np.dtype(SPACE_DTYPE[k])]
        for r in range(lo, hi):
            plan[r] = (blk << 16) | width[blk]
            width[blk] += 1
    assert width[0] == 8 and width[1] == 4 and sum(width) == F
    return F, tuple(width), plan


def _shuffled_plan(F, widths, seed):
    """Rows dealt to the blocks in a seeded order, every column of every block named once."""
    g = np.random.default_rng(seed)
    entries = [(blk << 16) | col for blk, w in enumerate(widths) for col in g.permutation(w)]
    assert len(entries) == F
    return np.asarray(entries, np.int32)[g.permutation(F)]


def _width_cases():
    F, widths, plan = _salad_widths()
    cases = {"salad": (F, widths, plan),
             "all_int8": (F, (0, 0, F), _shuffled_plan(F, (0, 0, F), 1)),
             "all_int64": (F, (F, 0, 0), _shuffled_plan(F, (F, 0, 0), 2)),
             "all_float32": (F, (0, F, 0), _shuffled_plan(F, (0, F, 0), 3)),
             # odd w8 (and odd n below): the int8 spans start 4- but not 16-byte aligned
             "odd_w8": (29, (8, 4, 17), _shuffled_plan(29, (8, 4, 17), 4)),
             # 203 * 8 + 3 * 4 + 1 + 24 bytes per env: a tile does not fit the kernel's LDS at once, it goes in passes
             "passes": (207, (203, 3, 1), _shuffled_plan(207, (203, 3, 1), 5))}
    return cases


def _rows(ot, F, n, seed):
    """[F][n] rows of the element type, negative values everywhere, int32 extremes (int64 columns
    must sign-extend them) and values outside +-127 (int8 columns must truncate them alike)."""
    g = np.random.default_rng(seed)
    if ot == 1:
        return torch.from_numpy(g.integers(-128, 128, (F, n)).astype(np.int8))
    v = g.integers(-70000, 70000, (F, n))
    pick = g.random((F, n))
    if ot == 0:
        v[pick < 0.05], v[pick > 0.95] = I32.min, I32.max
        v[(pick > 0.45) & (pick < 0.5)] = -129
        return torch.from_numpy(v.astype(np.int32))
    v[pick < 0.05], v[pick > 0.95] = -(1 << 24), 1 << 24            # integers a float32 holds exactly
    v[(pick > 0.45) & (pick < 0.5)] = 128
    return torch.from_numpy(v.astype(np.float32))


def _vectors(n, seed):
    g = np.random.default_rng(seed)
    return {"timestep": torch.from_numpy(g.integers(-5, 500, n).astype(np.float64)),
            "reward": torch.from_numpy(g.standard_normal(n) * 100),
            "ep_return": torch.from_numpy(g.standard_normal(n) * 1e6),
            "done": torch.from_numpy(g.integers(-2, 3, n).astype(np.int32)),
            "ep_length": torch.from_numpy(g.integers(-I32.max, I32.max, n).astype(np.int32))}


def _wait(ev):
    import time
    end = time.monotonic() + 30
    while not ev.query():
        assert time.monotonic() < end, "the pack did not finish"


@pytest.mark.parametrize("ot", [0, 1, 2], ids=["int32", "int8", "float32"])
@pytest.mark.parametrize("case", ["salad", "all_int8", "all_int64", "all_float32", "odd_w8", "passes"])
def test_tiled_pack_writes_the_bytes_of_the_plain_pack(case, ot):
    from gym_comm_amd.vec_env import MappedBuffer
    _lib, L = _lib_hostio()
    t = L.oc_pack_host_tile()
    F, (w64, w32, w8), plan = _width_cases()[case]
    plan_d = torch.from_numpy(plan).cuda()
    dev = torch.cuda.current_device()
    ns = [1, t - 1, t, t + 1, 3 * t + 17, 777]
    assert all(n >= 1 for n in ns) and len({(n + t - 1) // t for n in ns}) >= 4
    ev = torch.cuda.Event()
    for n in ns:
        rows = _rows(ot, F, n, 100 + n).cuda()
        vec = {k: v.cuda() for k, v in _vectors(n, 200 + n).items()}
        for optional in (True, False):
            total = L.oc_pack_host_bytes(w64, w32, w8, *([int(optional)] * 4), n)
            assert total > 0
            opt = lambda k: vec[k].data_ptr() if optional else None
            args = lambda out: (rows.data_ptr(), ot, F, plan_d.data_ptr(), w64, w32, w8, vec["timestep"].data_ptr(),
                                opt("reward"), opt("ep_return"), opt("done"), opt("ep_length"), out, n)
            want = torch.full((total + CANARY,), FILL, dtype=torch.uint8, device="cuda")
            got = torch.full((total + CANARY,), FILL, dtype=torch.uint8, device="cuda")
            _lib.call(L, "oc_pack_host", dev, *args(want.data_ptr()))
            _lib.call(L, "oc_pack_host_tiled", dev, *args(got.data_ptr()))
            want_h, got_h = want.cpu().numpy(), got.cpu().numpy()
            where = np.nonzero(want_h != got_h)[0]
            assert where.size == 0, (case, n, optional, total, where[:8].tolist())
            assert (want_h[total:] == FILL).all()                    # (the yardstick keeps to its bytes too)
            assert (want_h[:total] != FILL).any()
            # the same launch into host-mapped memory, read on the host once the event has completed
            buf = MappedBuffer(L, dev, total + CANARY)
            host = buf.view()
            assert host.base is buf and host.shape == (total + CANARY,) and host.dtype == np.uint8
            host[:] = FILL
            _lib.call(L, "oc_pack_host_tiled", dev, *args(buf.dev))
            ev.record(torch.cuda.current_stream())
            _wait(ev)
            where = np.nonzero(host != got_h)[0]
            assert where.size == 0, (case, n, optional, total, where[:8].tolist())
            del host, buf


def _arg(T=30):
    return SimpleNamespace(level="open-divider_salad", num_agents=2, max_num_timesteps=T, ego_config={},
                           partner_config={}, num_communication=3, communication_on=True, ego_led=False,
                           fow_radius=1)


def _owner(a):
    while isinstance(a, np.ndarray):
        a = a.base
    return a


def test_mapped_env_returns_what_the_copying_env_returns():
    """The shape of test_numpy_api_arrays_with_and_without_reused_host_buffers: 777 envs, T = 30,
    C = 3, 70 steps; a copying env, a mapped env and a mapped env with reused buffers agree in every
    observation array (values and declared dtypes), reward, done flag and episode info at every step."""
    from gym_comm_amd.vec_env import MappedBuffer, OvercookedVecEnv, SPACE_DTYPE
    n = 777
    vc = OvercookedVecEnv(_arg(), n, seed=3)
    vm = OvercookedVecEnv(_arg(), n, seed=3, host_io="mapped")
    vr = OvercookedVecEnv(_arg(), n, seed=3, host_io="mapped", reuse_host_buffers=True)
    oc, om, orr = vc.reset(), vm.reset(), vr.reset()
    for key in oc:
        assert np.array_equal(oc[key], om[key]) and np.array_equal(oc[key], orr[key]), key
        assert om[key].dtype == orr[key].dtype == np.dtype(SPACE_DTYPE[key]), key
    rng = np.random.default_rng(0)
    kept, last, episodes = [], None, 0
    for k in range(70):
        acts = np.stack([rng.integers(0, 4, n), rng.integers(0, 3, n)], axis=1)
        oc, rc, dc, ic = vc.step(acts)
        om, rm, dm, im = vm.step(acts)
        orr, rr, dr, ir = vr.step(acts)
        if last is not None:
            # a reused view of step k - 1 is untouched by step k, which wrote the other buffer -- and
            # step k did write something else (every env's timestep moves at every step)
            for key, (view, snapshot) in last.items():
                assert np.array_equal(view, snapshot), (k, key)
                now = rr if key == "rewards" else orr[key]
                assert not np.shares_memory(view, now), (k, key)
                assert _owner(view) is not _owner(now), (k, key)
            assert not np.array_equal(orr["timestep"], last["timestep"][1]), k
        assert sorted(oc) == sorted(om) == sorted(orr)
        for key in oc:
            assert om[key].dtype == orr[key].dtype == oc[key].dtype == np.dtype(SPACE_DTYPE[key]), key
            assert om[key].shape == orr[key].shape == oc[key].shape, key
            assert np.array_equal(oc[key], om[key]), (k, key)
            assert np.array_equal(oc[key], orr[key]), (k, key)
        assert rm.dtype == rr.dtype == np.float32 and dm.dtype == dr.dtype == bool
        assert np.array_equal(rc, rm) and np.array_equal(rc, rr)
        assert np.array_equal(dc, dm) and np.array_equal(dc, dr)
        for i in range(n):
            assert ic[i] == im[i] == ir[i], (k, i)
        episodes += sum("episode" in d for d in ic)
        kept.append((om["object_encodings_x"], om["object_encodings_x"].copy(), om["state_encodings"],
                     om["state_encodings"].copy()))
        last = {key: (orr[key], orr[key].copy()) for key in orr}
        last["rewards"] = (rr, rr.copy())
        assert isinstance(_owner(orr["timestep"]), MappedBuffer) and isinstance(_owner(rr), MappedBuffer)
        assert not isinstance(_owner(om["timestep"]), MappedBuffer)          # one host copy out of the buffer
    assert episodes >= 2 * n                # 70 steps of 30-step episodes
    for x, xs, s, ss in kept:               # fresh arrays stay what they were
        assert np.array_equal(x, xs) and np.array_equal(s, ss)
    # the single-launch path was taken, and its actions came from mapped memory
    assert vm._fast and vr._fast and isinstance(vm._io.act, MappedBuffer)
    assert vc._io.act is None
    # the mapped memory outlives the env while an array of it is alive, and goes with the last one
    owner = weakref.ref(_owner(orr["is_hidden"]))
    want = orr["is_hidden"].copy()
    del vr, last, rr, view, snapshot, now
    keep = orr["is_hidden"]
    del orr
    gc.collect()
    assert owner() is not None and np.array_equal(keep, want)
    del keep
    gc.collect()
    assert owner() is None


def test_mapped_env_on_the_slow_path_with_terminal_observations():
    from gym_comm_amd.vec_env import OvercookedVecEnv
    n = 130
    vc = OvercookedVecEnv(_arg(10), n, seed=5, terminal_obs=True)
    vm = OvercookedVecEnv(_arg(10), n, seed=5, terminal_obs=True, host_io="mapped")
    oc, om = vc.reset(), vm.reset()
    rng = np.random.default_rng(1)
    terminals = 0
    for k in range(25):
        acts = np.stack([rng.integers(0, 4, n), rng.integers(0, 3, n)], axis=1)
        oc, rc, dc, ic = vc.step(acts)
        om, rm, dm, im = vm.step(acts)
        for key in oc:
            assert oc[key].dtype == om[key].dtype and np.array_equal(oc[key], om[key]), (k, key)
        assert np.array_equal(rc, rm) and np.array_equal(dc, dm)
        for i in range(n):
            assert sorted(ic[i]) == sorted(im[i]), (k, i)
            if dc[i]:
                assert ic[i]["episode"] == im[i]["episode"]
                tc, tm = ic[i]["terminal_observation"], im[i]["terminal_observation"]
                assert sorted(tc) == sorted(tm)
                for key in tc:
                    assert tc[key].dtype == tm[key].dtype and np.array_equal(tc[key], tm[key]), (k, i, key)
                terminals += 1
    assert terminals >= 2 * n and vm._fast is False and vm._io.act is None


def test_step_async_and_step_wait_keep_their_protocol():
    from gym_comm_amd.vec_env import OvercookedVecEnv
    n = 130
    va = OvercookedVecEnv(_arg(), n, seed=7, host_io="mapped")
    vb = OvercookedVecEnv(_arg(), n, seed=7, host_io="mapped")
    va.reset(), vb.reset()
    rng = np.random.default_rng(2)
    with pytest.raises(RuntimeError):
        vb.step_wait()                                  # nothing was started
    for k in range(12):
        acts = np.stack([rng.integers(0, 4, n), rng.integers(0, 3, n)], axis=1)
        oa, ra, da, ia = va.step(acts)
        vb.step_async(acts)
        if k == 5:
            with pytest.raises(RuntimeError) as e:
                vb.step_async(acts)
            assert "step_wait" in str(e.value)          # and the step that was started is still there
        ob, rb, db, ib = vb.step_wait()
        for key in oa:
            assert np.array_equal(oa[key], ob[key]), (k, key)
        assert np.array_equal(ra, rb) and np.array_equal(da, db) and ia == ib
    with pytest.raises(RuntimeError):
        vb.step_wait()
