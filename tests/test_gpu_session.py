"""GPU: a real worker bound to an MI355X through the notebook path, RCCL data plane."""
import pytest

from nbdistributed_amd.session import Session

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu_session(require_gpu):
    s = Session(writer=lambda t: None)
    s.start(1, backend="auto", startup_timeout=600)
    yield s
    s.shutdown()


def test_ready_reports_mi355x(gpu_session):
    st = gpu_session.ready[0]
    assert st["cuda_available"]
    assert st["backend"] == "rccl"
    assert "gfx950" in st.get("gcn_arch", "")
    assert st["gpu_memory_total"] > 200  # GiB of HBM3E


def test_rccl_collectives_in_cell(gpu_session):
    code = (
        "x = torch.ones(1 << 20, device=device, dtype=torch.bfloat16)\n"
        "dist.all_reduce(x)\n"
        "y = [torch.empty(4, device=device) for _ in range(world_size)]\n"
        "dist.all_gather(y, torch.full((4,), float(rank), device=device))\n"
        "dist.broadcast(x, src=0)\n"
        "torch.cuda.synchronize()\n"
        "(x.float().sum().item(), dist.get_backend(), str(device))"
    )
    r = gpu_session.execute(code, render=False)
    out = r.results[0]["output"]
    assert "1048576.0" in out and "'rccl'" in out and "cuda:0" in out


def test_status_and_sync(gpu_session):
    st = gpu_session.status()
    assert st[0]["running"] and st[0]["cuda_available"]
    assert gpu_session.sync()[0]["status"] == "synced"


def test_cell_latency_on_gpu_worker(gpu_session):
    import time

    lat = []
    for _ in range(50):
        t = time.perf_counter()
        gpu_session.execute("1 + 1", render=False)
        lat.append(time.perf_counter() - t)
    lat.sort()
    assert lat[len(lat) // 2] < 0.005  # < 5 ms p50 (reference: 111.6 ms)


def test_plain_bench_run_loads_the_native_libraries(gpu_session, tmp_path):
    """bench.py's plain run on a GPU: exactly warm-up + steps trivial cells, the dump, then one last
    cell that loads the HIP library, checks a kernel's answer and reports what the rank has mapped."""
    import os

    import numpy as np

    from nbdistributed_amd import benchmarking as B

    ran, execute = [], gpu_session.execute
    gpu_session.execute = lambda code, *a, **kw: (ran.append(code), execute(code, *a, **kw))[1]
    try:
        res = B.run_all(gpu_session, 20, 2, allreduce=False, sweep=False, ddp=False, bcast=False, notebook=False,
                        checks=False, extras=False, dump_dir=str(tmp_path), native_probe=True)
    finally:
        del gpu_session.execute
    assert ran == ["1 + 1"] * 22 + [B.NATIVE_PROBE]  # 2 warm-up + 20 timed cells, then the probe; no other phase
    assert set(res) == {"cell", "native", "dumped_outputs"}
    line = B.result_line(res, 1, 20, 2)
    assert line["value"] > 0 and line["ms_per_step"] > 0 and "native_error" not in line
    libs = {os.path.basename(p) for p in line["native_libs"]["0"]}
    assert {"libnbd_ops.so", "libnbd_transport.so"} <= libs, line["native_libs"]
    assert (np.load(tmp_path / "cell_echo.npy") == np.array([2.0])).all()


def test_cell_gpu_time_reaches_the_timeline(gpu_session):
    # the end event is recorded after the reply and the time reported with a later cell
    code = ("a = torch.randn(4096, 4096, device=device)\n"
            "for _ in range(20):\n    a = (a @ a).tanh_()\n")
    gpu_session.execute(code, render=False)
    gpu_session.execute("torch.cuda.synchronize()", render=False)
    gpu_session.execute("1", render=False)
    recs = gpu_session.timeline.to_list()
    timed = [x for x in recs if "a @ a" in x["code_preview"] and x["per_rank"].get(0, {}).get("gpu_ms")]
    assert timed, recs[-3:]
    ms = timed[-1]["per_rank"][0]["gpu_ms"]
    assert 0.5 < ms < 60_000, ms  # 20 fp32 4096^3 products: milliseconds of GPU time


def test_nbd_ddp_on_gpu_matches_plain_backward(gpu_session):
    code = (
        "import copy\n"
        "from nbdistributed_amd.models import GPT2, GPT2Config\n"
        "from nbdistributed_amd.parallel import DistributedDataParallel as NbdDDP\n"
        "torch.manual_seed(0)\n"
        "base = GPT2(GPT2Config.tiny()).to(device)\n"
        "plain = copy.deepcopy(base)\n"
        "d32 = NbdDDP(copy.deepcopy(base), bucket_cap_mb=0.05, first_bucket_mb=0.01)\n"
        "d16 = NbdDDP(copy.deepcopy(base), comm_dtype=torch.bfloat16)\n"
        "idx = torch.randint(0, 512, (4, 64), device=device)\n"
        "for m in (plain, d32, d16):\n"
        "    m(idx, idx)[1].backward()\n"
        "torch.cuda.synchronize()\n"
        "e32 = max(float((p.grad - q.grad).abs().max()) for p, q in zip(plain.parameters(), d32.module.parameters()))\n"
        "e16 = max(float(((p.grad - q.grad).abs().max() / (p.grad.abs().max() + 1e-12))) "
        "for p, q in zip(plain.parameters(), d16.module.parameters()))\n"
        "(len(d32.buckets) > 1, e32 == 0.0, e16 < 1e-2)"
    )
    r = gpu_session.execute(code, render=False)
    assert r.results[0]["output"] == "(True, True, True)", r.results[0]


def test_tensor_echo_uses_device_summary(gpu_session):
    r = gpu_session.execute("big = torch.ones(1 << 20, device=device, dtype=torch.bfloat16) * 2\nbig", render=False)
    out = r.results[0]["output"]
    assert "mean=2" in out and "std=0" in out and "cuda:0" in out


def test_accelerate_on_rccl_backend(gpu_session):
    from test_accelerate import ACCEL

    r = gpu_session.execute(ACCEL, render=False)
    assert r.ok, r.errors
    assert r.results[0]["echo"].endswith("'cuda:0')"), r.results[0]


def test_flat_adamw_bf16_tracks_fp32_training(gpu_session):
    """GPT-2 tiny: bf16 params + FlatAdamW (fused HIP optimizer reading the DDP buckets) vs fp32
    params + autocast + torch fused AdamW: the loss curves agree."""
    code = (
        "import copy\n"
        "from nbdistributed_amd.models import GPT2, GPT2Config\n"
        "from nbdistributed_amd.parallel import DistributedDataParallel as NbdDDP\n"
        "from nbdistributed_amd.optim import FlatAdamW\n"
        "torch.manual_seed(0)\n"
        "base = GPT2(GPT2Config.tiny()).to(device)\n"
        "ref = NbdDDP(copy.deepcopy(base))\n"
        "oref = torch.optim.AdamW(ref.parameters(), lr=1e-3, fused=True)\n"
        "flat = NbdDDP(copy.deepcopy(base).to(torch.bfloat16), flat_params=True, grad_mode='bucket')\n"
        "oflat = FlatAdamW(flat, lr=1e-3)\n"
        "idx = torch.randint(0, 512, (4, 64), device=device)\n"
        "lr_, lf_ = [], []\n"
        "for i in range(30):\n"
        "    with torch.autocast('cuda', dtype=torch.bfloat16):\n"
        "        l1 = ref(idx, idx)[1]\n"
        "    l1.backward(); oref.step(); oref.zero_grad()\n"
        "    l2 = flat(idx, idx)[1]\n"
        "    l2.backward(); oflat.clip_grad_norm_(10.0); oflat.step()\n"
        "    lr_.append(float(l1.detach())); lf_.append(float(l2.detach()))\n"
        "(lr_[0], lr_[-1], lf_[0], lf_[-1])"
    )
    r = gpu_session.execute(code, render=False)
    r0, r1, f0, f1 = eval(r.results[0]["echo"])
    assert abs(r0 - f0) < 0.05 * r0, (r0, f0)  # same init, bf16 vs fp32-autocast forward
    assert r1 < r0 - 0.5, (r0, r1)             # memorising one batch: the loss falls
    assert abs(r1 - f1) < 0.1 * r1 + 0.1, (r1, f1)


GRAPH = """
from nbdistributed_amd.models import GPT2, GPT2Config
from nbdistributed_amd.parallel import DistributedDataParallel as NbdDDP
from nbdistributed_amd.optim import FlatAdamW
from nbdistributed_amd.graphs import GraphedStep
cfg = GPT2Config(vocab_size=1024, n_positions=256, n_embd=256, n_layer=2, n_head=4)
def build(capturable):
    torch.manual_seed(7)
    m = NbdDDP(GPT2(cfg).to(device, torch.bfloat16), flat_params=True, grad_mode="bucket")
    return m, FlatAdamW(m, lr=1e-3, capturable=capturable)
g = torch.Generator().manual_seed(1)
xs = [torch.randint(0, 1024, (2, 256), generator=g).to(device) for _ in range(6)]
def make_step(m, o):
    def step(x):
        loss = m(x, x, return_logits=False)[1]
        loss.backward()
        o.clip_grad_norm_(1.0)
        o.step()
        o.zero_grad()
        return loss.detach()
    return step
m1, o1 = build(False)
s1 = make_step(m1, o1)
for _ in range(2):
    s1(xs[0])                      # the graphed run's warm-up steps
eager = []
for i, x in enumerate(xs[1:]):
    if i == 3:
        o1.param_groups[0]["lr"] = 5e-4
    eager.append(float(s1(x)))
m2, o2 = build(True)
gs = GraphedStep(make_step(m2, o2), (xs[0],), warmup=2, optimizers=[o2])
graphed = []
for i, x in enumerate(xs[1:]):
    if i == 3:
        o2.param_groups[0]["lr"] = 5e-4
    graphed.append(float(gs(x)))
torch.cuda.synchronize()
perr = max(float((a.float() - b.float()).abs().max()) for a, b in zip(m1.module.parameters(), m2.module.parameters()))
lerr = max(abs(a - b) for a, b in zip(eager, graphed))
(perr < 1e-2, lerr < 1e-2, gs.replays, int(o2.step_t.item()))
"""


def test_graphed_training_step_matches_eager(gpu_session):
    """HIP-graph capture of a whole DDP step (fwd, bwd, bucket flatten + RCCL all-reduce on the
    side stream, device-side clip, capturable FlatAdamW) from a notebook cell."""
    r = gpu_session.execute(GRAPH, render=False, raise_on_error=False)
    assert r.ok, r.errors
    assert r.results[0]["echo"] == "(True, True, 5, 7)", r.results[0]


def test_status_reports_block_graph_activity(gpu_session):
    """%dist_status's per-rank block-graph line: the worker reports the per-block / stack graph
    counters once the native ops are loaded."""
    code = """
from nbdistributed_amd import ops
from nbdistributed_amd.models.llama import LlamaConfig, LlamaForSequenceClassification
torch.manual_seed(0)
_m = LlamaForSequenceClassification(LlamaConfig.smollm2_135m(num_hidden_layers=2)).to(device, torch.bfloat16)
_m.model.block_graphs = 1
_ids = torch.randint(1, 49152, (2, 128), device=device)
for _ in range(8):
    _m(_ids, torch.ones_like(_ids), torch.tensor([0, 1], device=device))[0].backward()
torch.cuda.synchronize()
ops.block_graphs_stats()["stack_replays"]
"""
    r = gpu_session.execute(code, render=False)
    assert r.ok, r.errors
    assert int(r.results[0]["echo"]) >= 1, r.results[0]
    st = gpu_session.status()
    bg = st[0].get("block_graphs")
    assert bg is not None and bg["stack_replays"] >= 1 and bg["captures"] >= 2, bg
    gpu_session.execute("del _m\nimport gc; gc.collect()", render=False)
