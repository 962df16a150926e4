"""Multi-process (gloo, world_size 2 / 4 / 8, CPU) tests of the exchange of the multi-GPU step:
sum all-reduce of gradient ranges (fp32 / fp16 / bf16 wire), MAX reduction of the occupancy-grid estimates, and the
sharded form -- reduce-scatter of a wire buffer of `world` chunks with flag slots, in-place all-gather of the owners'
slices -- plus the ray-sharding helpers and the bf16 summation drift of an 8-way reduction."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, tmp):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from nerf_vo_amd.parallel import GradientAllReduce

    checks = {}
    red = GradientAllReduce(dist, bucket_numel=1000)
    g = torch.Generator().manual_seed(100 + rank)
    n = 10_007  # not a multiple of the bucket size
    grad = torch.randn(n, generator=g)
    mine = grad.clone()
    red(grad)
    # every rank must hold the same sum; checked against a locally recomputed reference (summation order differs)
    gathered = [torch.zeros(n) for _ in range(world)]
    dist.all_gather(gathered, mine)
    ref = sum(gathered)
    checks["fp32 all-reduce"] = torch.allclose(grad, ref, atol=2e-6 * world)
    # partial reduction: only one segment is reduced, the rest keeps the local value
    grad2 = mine.clone()
    red(grad2, segments=[(100, 2500)])
    checks["segment all-reduce"] = torch.allclose(grad2[100:2600], ref[100:2600], atol=2e-6 * world) and \
        torch.equal(grad2[:100], mine[:100]) and torch.equal(grad2[2600:], mine[2600:])
    # 2-byte wires: every rank's contribution is rounded once, and the collective rounds the running sum to the wire
    # format after every add -- the bound grows with the number of adds
    adds = world - 1
    red16 = GradientAllReduce(dist, bucket_numel=3000, compress="fp16")
    grad3 = mine.clone()
    red16(grad3, segments=[(0, 5000), (5000, n - 5000)])
    ref16 = sum(t.half().float() for t in gathered)
    checks["fp16 wire"] = torch.allclose(grad3, ref16, atol=1e-2 * adds, rtol=2e-3 * adds)
    # bf16-compressed exchange (what bench.py uses): 8 significant bits, fp32's exponent range -- tiny values survive
    redb = GradientAllReduce(dist, compress="bf16")
    tiny = mine.clone() * 1e-12
    back = redb(tiny.clone(), keep_half=True)
    refb = sum((t * 1e-12).to(torch.bfloat16).float() for t in gathered)
    checks["bf16 wire keeps tiny values"] = back.dtype == torch.bfloat16 and \
        torch.allclose(back.float(), refb, rtol=1e-2 * adds, atol=4e-14 * adds) and float((back.float() == 0).float().mean()) < 1e-3
    # asynchronous form (the multi-GPU step overlaps the fields reduction with the next sampling prefix): handles out,
    # same sum after wait(); compressed variant through the caller-owned 2-byte buffer
    grad4 = mine.clone()
    handles = red(grad4, segments=[(0, n)], async_op=True)
    red.wait(handles)
    checks["async all-reduce"] = len(handles) > 0 and torch.allclose(grad4, ref, atol=2e-6 * world)
    half = mine.to(torch.bfloat16)
    handles = redb.reduce_half(mine, half, [(0, 4000), (6000, n - 6000)], already_cast=True, async_op=True)
    redb.wait(handles)
    refh = sum(t.to(torch.bfloat16).float() for t in gathered)
    checks["async bf16 reduce_half"] = torch.allclose(half[:4000].float(), refh[:4000], rtol=1e-2 * adds, atol=4e-2 * adds) and \
        torch.equal(half[4000:6000], mine[4000:6000].to(torch.bfloat16))
    # MAX reduction of the occupancy-grid density estimates: identical on every rank, elementwise maximum
    dens = mine.abs().clone()
    red.reduce_max(dens)
    checks["max reduction"] = torch.equal(dens, torch.stack([t.abs() for t in gathered]).max(dim=0).values)
    # sharded exchange: reduce-scatter of a wire buffer of `world` chunks (+ flag slots), all-gather of the owners' slices
    # IN PLACE (the shard is a slice of the full buffer, as the optimiser writes it)
    reds = GradientAllReduce(dist, compress="bf16", shard_optimizer=True)
    per, pad = 1000, 8
    wire = torch.zeros(world * (per + pad), dtype=torch.bfloat16)
    for c in range(world):
        wire[c * (per + pad):c * (per + pad) + per] = mine[c * per:(c + 1) * per].to(torch.bfloat16)
        wire[c * (per + pad) + per:(c + 1) * (per + pad)] = 1.0 if rank % 4 == 1 else 0.0  # ranks 1, 5 "overflowed"
    out = torch.zeros(per + pad, dtype=torch.bfloat16)
    reds.wait(reds.reduce_scatter(out, wire, async_op=True))
    ref_chunk = sum(t[rank * per:(rank + 1) * per].to(torch.bfloat16).float() for t in gathered)
    # every rank finds the NUMBER of ranks that overflowed in the flag slots of its own chunk: all ranks skip together
    n_bad = len([r for r in range(world) if r % 4 == 1])
    checks["reduce-scatter values"] = torch.allclose(out[:per].float(), ref_chunk, rtol=1e-2 * adds, atol=4e-2 * adds)
    checks["reduce-scatter flag slots"] = bool((out[per:] == float(n_bad)).all())
    full = torch.zeros(world * per, dtype=torch.bfloat16)
    full[rank * per:(rank + 1) * per] = out[:per]
    reds.wait(reds.all_gather(full, full[rank * per:(rank + 1) * per], async_op=True))
    chunks = [torch.zeros(per, dtype=torch.bfloat16) for _ in range(world)]
    dist.all_gather(chunks, out[:per].clone())
    checks["in-place all-gather"] = torch.equal(full, torch.cat(chunks)) and reds.world == world and reds.rank == rank
    try:
        GradientAllReduce(dist, shard_optimizer=True)
        checks["sharding needs a 2-byte wire"] = False
    except ValueError:
        checks["sharding needs a 2-byte wire"] = True
    torch.save({k: bool(v) for k, v in checks.items()}, os.path.join(tmp, f"r{rank}.pt"))
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4, 8])
def test_gradient_exchange_gloo(tmp_path, world):
    port = _free_port()
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    for r in range(world):
        checks = torch.load(tmp_path / f"r{r}.pt")
        bad = [k for k, v in checks.items() if not v]
        assert len(checks) == 11 and not bad, f"world {world}, rank {r}: {bad}"


def test_single_process_world_is_identity():
    from nerf_vo_amd.parallel import GradientAllReduce, shard_ray_count

    class _NoDist:
        @staticmethod
        def is_initialized():
            return False

    red = GradientAllReduce(_NoDist())
    x = torch.arange(10.0)
    y = x.clone()
    red(y)
    assert torch.equal(x, y)
    assert [shard_ray_count(4096, 8, r) for r in range(8)] == [512] * 8
    assert sum(shard_ray_count(4099, 8, r) for r in range(8)) == 4099


def test_fields_shards_split_evenly_for_every_world_size():
    """Slice arithmetic of the sharded optimiser (engine._capture_step / optimizer_step: per = (f_hi - f_lo) // world,
    chunks of the wire buffer = per + 8 flag slots): the fields group is padded to a multiple of 512 elements
    (engine: 'field.pad'), so that for world 1 / 2 / 4 / 8 the shards are equal, 16-byte aligned in the 2-byte wire
    format and in the fp32 master, and tile the group exactly."""
    n_base, n_color, n_emb = 12_199_312, 9216, 192 * 32  # base MLP + main grid | colour head | embedding (192 keyframes)
    off = n_base + n_color + n_emb
    fields = off + (-off) % 512
    for world in (1, 2, 4, 8):
        per = fields // world
        assert per * world == fields and per % 8 == 0 and (2 * per) % 16 == 0 and (4 * per) % 16 == 0
        kPad = 8
        starts = [r * (per + kPad) for r in range(world)]
        assert all((2 * s) % 16 == 0 for s in starts)  # every chunk of the wire buffer starts 16-byte aligned
        covered = sum(per for _ in range(world))
        assert covered == fields


def test_bf16_wire_summation_drift_up_to_eight_ranks():
    """RCCL sums the 2-byte wire format in that format: an 8-rank ring rounds the running sum to bf16's 8 significant bits
    seven times where two ranks round once.  Emulated here as a sequential bf16 accumulation of per-rank gradients
    (heavy-tailed magnitudes, as hash-grid gradients are) against the exact sum: the relative L1 error of the reduced
    gradient grows from 1.9e-3 (W = 2) to 3.2e-3 (W = 8) -- 1.7x, below the 2x at which DESIGN.md section 6 would switch
    the reduction to fp32 after a bf16 all-gather (which measures 1.5e-3 at every W, also checked)."""
    g = torch.Generator().manual_seed(0)
    n = 400_000
    err = {}
    for world in (2, 4, 8):
        grads = [torch.randn(n, generator=g) * torch.rand(n, generator=g).pow(4) * 1e-3 for _ in range(world)]
        ref = sum(t.double() for t in grads)
        acc = grads[0].to(torch.bfloat16)
        for t in grads[1:]:
            acc = acc + t.to(torch.bfloat16)
        wide = sum(t.to(torch.bfloat16).float() for t in grads)
        err[world] = (float((acc.double() - ref).abs().sum() / ref.abs().sum()),
                      float((wide.double() - ref).abs().sum() / ref.abs().sum()))
    print({w: tuple(f"{v:.2e}" for v in e) for w, e in err.items()})
    assert err[2][0] < 2.5e-3 and err[8][0] < 4.5e-3
    assert err[8][0] < 2.0 * err[2][0], "8-way bf16 addition drifts more than twice the 2-way figure"
    assert all(e[1] < 2.0e-3 for e in err.values())


def test_bench_launches_its_own_ranks(tmp_path):
    """`python bench.py --gpus 2` as the driver types it for N = 1 (no launcher around it): the process starts its two
    ranks itself, relays rank 0's single JSON line and returns the job's exit code.  NVO_BENCH_DRY=1 keeps the ranks
    off the GPU (gloo rendezvous + the max-over-ranks reduction only), so the whole entry path runs here."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, NVO_BENCH_DRY="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    res = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1"],
                         capture_output=True, text=True, env=env, timeout=300, cwd=str(tmp_path))
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, res.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["warmup"] == 1 and out["max_over_ranks"] == 2.0


def test_bench_names_the_error_when_the_node_has_too_few_gpus(tmp_path):
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "NVO_BENCH_DRY")}
    res = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "64"], capture_output=True, text=True,
                         env=env, timeout=300, cwd=str(tmp_path))
    assert res.returncode == 3 and "not-enough-gpus" in res.stderr and res.stdout.strip() == ""


def test_bench_dump_outputs_is_seeded_and_bounded(tmp_path):
    """`bench.py --dump-outputs DIR`: the step's rendered rays as float32 and its loss terms as float64, whole up to
    DUMP_MAX_ROWS rows, a larger ray batch as the SAME seeded sample on every call, the dump below 64 MB."""
    import os
    import sys

    import numpy as np
    import torch

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench

    for R in (256, bench.DUMP_MAX_ROWS + 4096):
        class Engine:  # the attributes dump_outputs reads
            ws = {"out_rgb": torch.rand(R, 3), "out_depth": torch.rand(R), "out_expected_depth": torch.rand(R),
                  "out_accumulation": torch.rand(R)}

            def _workspace(self, R_, training):
                assert R_ == R and training
                return self.ws

            def loss_totals(self):
                return torch.arange(8, dtype=torch.float32)

        eng = Engine()
        for d in ("a", "b"):
            bench.dump_outputs(str(tmp_path / f"{R}{d}"), eng, R)
        names = sorted(os.listdir(tmp_path / f"{R}a"))
        assert names == sorted(f"{n}.npy" for n in ("rgb", "depth", "expected_depth", "accumulation", "losses"))
        total = 0
        for n in names:
            a, b = np.load(tmp_path / f"{R}a" / n), np.load(tmp_path / f"{R}b" / n)
            assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), n
            total += os.path.getsize(tmp_path / f"{R}a" / n)
        rgb = np.load(tmp_path / f"{R}a" / "rgb.npy")
        if R <= bench.DUMP_MAX_ROWS:
            assert np.array_equal(rgb, eng.ws["out_rgb"].numpy())
        else:
            assert rgb.shape == (bench.DUMP_MAX_ROWS, 3) and np.isin(rgb[:, 0], eng.ws["out_rgb"][:, 0].numpy()).all()
        assert np.load(tmp_path / f"{R}a" / "losses.npy").dtype == np.float64
        assert total < 64 << 20
