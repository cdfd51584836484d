"""CPU-only checks (run with -m "not gpu"): the C-ABI library loads and exports every symbol the header declares,
the drop-in module surface keeps the reference's constructor / state-dict contract, host-side step helpers match
the golden tables, and the data-parallel bucket logic works over gloo with world_size 2."""
import os
import re
import socket

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    import ctypes
    from transformertts_amd import _lib
    hdr = open(os.path.join(REPO, "include", "ttts_hip.h")).read()
    declared = set(re.findall(r"\b(ttts_[a-z0-9_]+)\s*\(", hdr))
    assert declared, "no declarations found"
    lib = _lib.load()                      # raises if the .so is missing: there is no fallback
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in ttts_hip.h but not exported"
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    assert lib.ttts_abi_version() >= 14
    # size queries are pure host functions: callable without a GPU
    assert lib.ttts_wgrad_workspace_bytes(55680, 256, 256, 5) > 0
    assert lib.ttts_layernorm_bwd_workspace_bytes(256) > 0
    # so is the one host-side object of the ABI, the caller-owned reduction queue
    q = lib.ttts_reduce_queue_create()
    assert q and lib.ttts_reduce_queue_pending(q) == 0 and lib.ttts_reduce_queue_clear(q) == 0
    lib.ttts_reduce_queue_destroy(q)


def test_library_keeps_no_hidden_configuration():
    """The product library reads no environment variables (round 2 had development knobs behind getenv) and keeps no
    process-wide queue: checked on the sources and on the built object's imports."""
    import glob
    import subprocess
    for src in glob.glob(os.path.join(REPO, "transformertts_amd", "csrc", "*")):
        assert "getenv" not in open(src).read(), src
    from transformertts_amd import _lib
    syms = subprocess.run(["nm", "-D", "--undefined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert "getenv" not in syms
    # ... and neither does the Python layer select arithmetic from the process environment (round 3 read TTTS_*_MODE at import
    # time): the only environment reads of the package are the library path of a development A/B build and the compiler name.
    allowed = {("_lib.py", "TTTS_LIB"), ("build.py", "HIPCC")}
    for path in glob.glob(os.path.join(REPO, "transformertts_amd", "**", "*.py"), recursive=True):
        for m in re.finditer(r"os\.environ(?:\.get\(|\[)\s*[\"']([A-Z_0-9]+)", open(path).read()):
            assert (os.path.basename(path), m.group(1)) in allowed, (path, m.group(1))


def test_bench_workload_is_the_oracles_workload():
    """bench.py and the launchers draw configurations and synthetic batches from transformertts_amd/workload.py (the product
    path must not import oracle/); the parity tests draw them from oracle/spec.py / oracle/synth.py.  The two copies must
    stay the same thing."""
    from oracle import spec, synth
    from transformertts_amd import workload
    for name in ("base", "scaled", "tiny", "micro", "tiny_k37"):
        assert workload.model_config(name) == spec.model_config(name), name
    for kw in (dict(B=4, Tp=100, Tm=870, ragged=False, seed=1234), dict(B=7, Tp=60, Tm=300, ragged=True, seed=5),
               dict(B=3, Tp=12, Tm=40, n_mels=16, n_phon=30, ragged=True, seed=21)):
        a, b = workload.synth_batch(**kw), synth.synth_batch(**kw)
        assert a.keys() == b.keys()
        for k in a:
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), (kw, k)


def test_error_path_without_gpu():
    """Argument validation happens before any launch and reports through ttts_last_error()."""
    from transformertts_amd import _lib
    lib = _lib.load()
    rc = lib.ttts_linear_fwd(None, None, None, None, None, 10, 16, 16, 0, 0.0, 0, None, 0, 0, None)
    assert rc == -1 and "null pointer" in _lib.last_error()
    with pytest.raises(RuntimeError):
        _lib.check(rc, "ttts_linear_fwd")


def test_product_path_rejects_cpu_tensors():
    from transformertts_amd import ops
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.linear(torch.zeros(4, 16), torch.zeros(16, 16))


def test_state_dict_contract_and_ctor_signature():
    import inspect
    from oracle.spec import model_config, state_spec
    from transformertts_amd.model import TransformerTTS
    for name in ("base", "tiny", "scaled", "micro", "tiny_k37"):
        cfg = model_config(name)
        m = TransformerTTS(**cfg, device="cpu")
        sd, spec = m.state_dict(), state_spec(cfg)
        assert list(sd.keys()) == list(spec.keys())
        assert all(tuple(sd[k].shape) == tuple(spec[k]) for k in spec)
    base = TransformerTTS(**model_config("base"), device="cpu")
    assert sum(p.numel() for p in base.parameters()) == 7904834
    assert len(base.state_dict()) == 159
    params = list(inspect.signature(TransformerTTS.__init__).parameters)[1:]
    assert params == ["encoder_prenet_n_layers", "encoder_prenet_in_channel", "encoder_prenet_out_channel",
                      "encoder_prenet_kernel_size", "encoder_prenet_dropout", "encoder_n_layers", "encoder_n_head",
                      "encoder_d_ffn", "encoder_dropout", "decoder_n_layers", "decoder_n_head", "decoder_d_ffn",
                      "decoder_dropout", "postnet_n_layers", "postnet_kernel_size", "postnet_dropout", "d_model",
                      "n_phon", "n_mels", "device"]
    fwd = inspect.signature(TransformerTTS.forward).parameters
    assert list(fwd)[1:5] == ["phoneme", "melspec", "phoneme_lens", "melspec_lens"]
    assert all(p.default is not inspect.Parameter.empty for p in list(fwd.values())[5:])   # extensions are optional
    # encoder layers start as identical deep copies (torch nn.TransformerEncoder semantics)
    assert torch.equal(base.encoder.layers[0].linear1.weight, base.encoder.layers[2].linear1.weight)


def test_step_helpers_match_golden(golden_dir):
    from transformertts_amd.utils.util import get_teacher_forcing_ratio, get_noam_scheduler
    g = np.load(os.path.join(golden_dir, "helpers.npz"))
    for mode in ("linear", "cosine", "constant"):
        got = [get_teacher_forcing_ratio(int(e), 300, mode, cycles=1) for e in g["tf/epochs"]]
        assert np.allclose(got, g[f"tf/{mode}"], rtol=0, atol=1e-15)
    with pytest.raises(ValueError):
        get_teacher_forcing_ratio(50, 300, "bogus")
    lam = get_noam_scheduler(256, 4000)
    assert np.allclose([lam(int(s)) for s in g["noam/steps"]], g["noam/256_4000"], rtol=1e-14)


def test_loss_mix_and_optimizer_have_no_cpu_path():
    """The product package holds no second (CPU / stock-torch) backend: the loss, the scheduled-sampling mix and the
    optimizer reject host tensors instead of computing with torch ops (the CPU restatement is oracle/, test-only)."""
    from transformertts_amd.loss import TransformerTTSLoss
    from transformertts_amd.optim import FlatAdam
    from transformertts_amd.utils.util import apply_teacher_forcing
    x = torch.zeros(2, 5, 8)
    lens = torch.tensor([5, 3])
    with pytest.raises(ValueError, match="no CPU fallback"):
        TransformerTTSLoss(8.0)({"pred_melspec": x, "post_melspec": x, "pred_stop": torch.zeros(2, 5)}, x, lens)
    with pytest.raises(ValueError, match="no CPU fallback"):
        apply_teacher_forcing(x, x, lens, 0.5)
    with pytest.raises(ValueError, match="no CPU"):
        FlatAdam([torch.nn.Parameter(torch.zeros(4))])
    import inspect
    import transformertts_amd.loss as L
    import transformertts_amd.utils.util as U
    import transformertts_amd.lightning_module as M
    for mod in (L, U, M):
        src = inspect.getsource(mod)
        assert "torch.optim.Adam(" not in src and "binary_cross_entropy" not in src and "max_pool1d" not in src


def test_reference_import_lines_bind_to_this_package(tmp_path):
    """The import lines of the reference's step surface (lightning_module.py:7-14, train.py:6-8) work verbatim with the
    repository root on sys.path and resolve to the MI355X-native implementation."""
    import importlib
    import subprocess
    import sys
    code = (
        "from model import TransformerTTS\n"
        "from loss import TransformerTTSLoss\n"
        "from utils.util import prepare_batch, get_noam_scheduler, apply_teacher_forcing, get_teacher_forcing_ratio\n"
        "from dataset import DataModule\n"
        "from lightning_module import LightningModule\n"
        "from utils.util import increment_path, setup_logger\n"
        "from utils.plot import (plot_mels_batch, plot_mels_single, plot_mels_scheduled, plot_alignments_batch,"
        " plot_alignment_single)\n"
        "from model.layers import TransformerDecoderLayer, TransformerDecoder\n"
        "from model.module import ConvNormBN, LinearNorm\n"
        "import transformertts_amd.model as m, transformertts_amd.loss as l\n"
        "assert TransformerTTS is m.TransformerTTS and TransformerTTSLoss is l.TransformerTTSLoss\n"
        f"p = increment_path(r'{tmp_path}'); import os; assert os.path.isdir(os.path.join(p, 'mels_scheduled'))\n"
        f"q = increment_path(r'{tmp_path}'); assert os.path.basename(q).startswith('exp_2_')\n"
        "import torch\n"
        "a = [torch.rand(3, 2, 12, 7).softmax(-1) for _ in range(2)]\n"
        "w = [plot_mels_batch(torch.rand(3, 12, 16), torch.rand(3, 10, 16), 1, p),"
        " plot_mels_scheduled(torch.rand(3, 12, 16), torch.rand(3, 12, 16), 1, p),"
        " plot_mels_single(torch.rand(12, 16), torch.rand(9, 16), 1, p),"
        " plot_alignments_batch(a, 1, p), plot_alignment_single(a, 2, 1, p)]\n"
        "names = ['mels_batch/valid_epoch_1.png', 'mels_scheduled/scheduled_epoch_1.png', 'mels_single/infer_epoch_1.png',"
        " 'align_batch/valid_align_batch_epoch_1.png', 'align_single/valid_align_2_epoch_1.png']\n"
        "assert all(x is None or (os.path.getsize(x) > 0 and x == os.path.join(p, n)) for x, n in zip(w, names)), w\n"
        "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]


def test_synth_batch_honours_collate_contract():
    from oracle.synth import synth_batch
    b = synth_batch(16, 100, 870, ragged=True, seed=3)
    pl, ml = b["phoneme_lens"], b["melspec_lens"]
    assert b["phoneme"].dtype == torch.int64 and b["melspec"].dtype == torch.float32 and pl.dtype == torch.int64
    assert torch.all(pl[:-1] >= pl[1:])                                     # sorted by phoneme length, descending
    assert b["phoneme"].shape == (16, int(pl.max())) and b["melspec"].shape == (16, int(ml.max()), 80)
    for i in range(16):
        assert torch.all(b["phoneme"][i, pl[i]:] == 0) and torch.all(b["melspec"][i, ml[i]:] == 0)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(rank, world, port, ret):
    import torch.distributed as dist
    from transformertts_amd.parallel import FlatGradBucket, broadcast_module_state, shard_batch
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.manual_seed(100 + rank)                      # replicas start different ...
        net = torch.nn.Sequential(torch.nn.Linear(12, 7), torch.nn.Tanh(), torch.nn.Linear(7, 3))
        broadcast_module_state(net)                        # ... and are made identical
        bucket = FlatGradBucket(net.parameters())
        g = torch.Generator().manual_seed(7)
        x, y = torch.randn(8, 12, generator=g), torch.randn(8, 3, generator=g)
        per = 8 // world
        bucket.zero()
        loss = ((net(x[rank * per:(rank + 1) * per]) - y[rank * per:(rank + 1) * per]) ** 2).mean()
        loss.backward()
        assert all(p.grad.data_ptr() == v.data_ptr() for p, v in zip(bucket.params, bucket.views))
        bucket.allreduce_mean()
        norm = bucket.clip_grad_norm_(1e9)
        # oracle: mean over ranks of per-shard mean gradients == gradient of the mean of per-shard losses
        ref = torch.nn.Sequential(torch.nn.Linear(12, 7), torch.nn.Tanh(), torch.nn.Linear(7, 3))
        ref.load_state_dict(net.state_dict())
        tot = sum(((ref(x[r * per:(r + 1) * per]) - y[r * per:(r + 1) * per]) ** 2).mean() for r in range(world)) / world
        tot.backward()
        for p, q in zip(net.parameters(), ref.parameters()):
            assert torch.allclose(p.grad, q.grad, atol=1e-6), "averaged gradient mismatch"
        flat_ref = torch.cat([q.grad.flatten() for q in ref.parameters()])
        assert abs(float(norm) - float(flat_ref.norm())) < 1e-5
        # overlapped form: the tail (second Linear) is reduced as soon as backward has left it, while the first Linear's
        # gradients are still being computed; the result is the same mean gradient.  The boundary module is called with
        # KEYWORD arguments only, the way the reference calls its decoder (model/model.py:298-306): a module-level full
        # backward hook would fire before the boundary's own parameter gradients exist in that case.
        from transformertts_amd.parallel import overlap_tail_with_backward

        class Kw(torch.nn.Module):
            def __init__(self, inner):
                super().__init__()
                self.inner = inner

            def forward(self, *, x):
                return self.inner(x)

        class Net(torch.nn.Module):
            def __init__(self, seq):
                super().__init__()
                self.a, self.act, self.b = seq[0], seq[1], Kw(seq[2])

            def forward(self, x):
                return self.b(x=self.act(self.a(x)))

        wrapped = Net(net)
        want = bucket.flat.clone()
        bucket.zero()
        lo = bucket.offset_of(net[2].weight)
        assert lo > 0
        seen_at_fire = []
        trig = overlap_tail_with_backward(
            bucket, wrapped, wrapped.b,
            on_ready=lambda lo_: (seen_at_fire.append(bucket.flat[lo_:].clone()), bucket.start_tail_allreduce(lo_))[1])
        assert trig is not None and trig.lo == lo
        with torch.no_grad():                           # a no-grad forward must not arm the trigger
            wrapped(x[:2])
        loss = ((wrapped(x[rank * per:(rank + 1) * per]) - y[rank * per:(rank + 1) * per]) ** 2).mean()
        local = torch.autograd.grad(loss, list(net[2].parameters()), retain_graph=True)
        loss.backward()
        assert trig.fired == 1 and len(seen_at_fire) == 1
        # the tail was complete when the trigger fired: it held exactly this rank's local gradients of the boundary
        assert torch.equal(seen_at_fire[0][:local[0].numel()], local[0].flatten())
        bucket.finish_allreduce()
        assert torch.allclose(bucket.flat, want, atol=1e-7)
        trig.remove()
        # a boundary that does not start the bucket's tail (or is not a child) is refused
        assert overlap_tail_with_backward(bucket, wrapped, wrapped.a) is None
        bucket.zero()                                   # without a started tail, finish == plain all-reduce
        loss = ((net(x[rank * per:(rank + 1) * per]) - y[rank * per:(rank + 1) * per]) ** 2).mean()
        loss.backward()
        bucket.finish_allreduce()
        assert torch.allclose(bucket.flat, want, atol=1e-7)
        batch = {"phoneme": torch.arange(40).view(4, 10), "melspec": torch.zeros(4, 9, 2),
                 "phoneme_lens": torch.tensor([10, 8, 6, 4]), "melspec_lens": torch.tensor([9, 7, 5, 3])}
        sh = shard_batch(batch, rank, world)
        assert sh["phoneme"].shape == (2, [10, 6][rank]) and sh["melspec"].shape == (2, [9, 5][rank], 2)
        ret[rank] = "ok"
    finally:
        dist.destroy_process_group()


def test_data_parallel_bucket_gloo_world2():
    import torch.multiprocessing as mp
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_dp_worker, args=(2, _free_port(), ret), nprocs=2, join=True)
    assert dict(ret) == {0: "ok", 1: "ok"}


def test_bench_starts_its_own_ranks_when_no_launcher_did():
    """`python bench.py --gpus 2` with no RANK / WORLD_SIZE in the environment (how a driver that only knows the 1-GPU command
    shape would call it) must start `torch.distributed.run --nproc-per-node 2` as a child, and rank 0 must print exactly ONE
    JSON line with n_gpus = 2.  --launch-check keeps the model and the GPU out of it (gloo on the host): the protocol around
    the step -- rendezvous on 127.0.0.1, barriers, MAX-over-ranks clock, SUM of units -- is what runs.  The same bare command
    with the real step is covered on the GPU box by test_two_rank_rehearsal_reduces_to_the_mean_gradient."""
    import json
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    r = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--launch-check"],
                       env=env, capture_output=True, text=True, timeout=300, cwd=repo)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["launch_check"] is True and out["steps"] == 3
    assert out["frames_per_step"] == 2 * 64 * 870          # SUM over ranks (weak scaling: 64 utterances per rank)
    # a failing child must fail the parent: an unknown flag makes every rank exit 2
    r = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--gpus", "2", "--no-such-flag"], env=env, capture_output=True,
                       text=True, timeout=300, cwd=repo)
    assert r.returncode != 0


def test_no_sgpr_hazard_in_front_of_inline_assembly_memory_instructions():
    """hipcc's hazard recogniser does not look inside inline assembly: a vector-memory instruction in an `asm` block that reads
    an SGPR a VALU instruction wrote fewer than 5 wait states earlier reads a stale value (tools/isa_hazard_scan.py).  Scans the
    gfx950 ISA of every kernel file that carries inline assembly (cross-compiles here, no GPU)."""
    import shutil
    import subprocess
    import sys
    if shutil.which(os.environ.get("HIPCC", "hipcc")) is None:
        pytest.skip("hipcc not on PATH")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "isa_hazard_scan.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    # and the scanner does find the pattern when it is there
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import isa_hazard_scan
    finally:
        sys.path.pop(0)
    isa = ["\tv_readlane_b32 s6, v137, 11", "\t;;#ASMSTART", "\tbuffer_load_dwordx4 v[46:49], v82, s[28:31], s6 offen", "\t;;#ASMEND"]
    assert len(isa_hazard_scan.scan(isa)) == 1
    isa.insert(1, "\ts_nop 4")
    assert isa_hazard_scan.scan(isa) == []


def test_dropout_seed_stream_restarts_with_a_reseeded_module():
    """train.py:24-28 of the reference seeds everything and then builds the module: doing that twice in one process with the
    same seed must give the same dropout masks (the reference draws them from torch's generator, which the seed resets).  Here
    the mask stream is `ops.seeds`; `torch.manual_seed(s)` with an unchanged s leaves torch.initial_seed() as it was, so the calls
    are counted (ops._torch_seed_calls) and a re-seed restarts the stream.  Building a module WITHOUT seeding again (evaluation
    copy, EMA / teacher, load_from_checkpoint) does not: the training module must not replay the masks of step 0.
    An explicit `manual_seed` pins the stream until `follow_torch()`."""
    from transformertts_amd import ops
    from transformertts_amd.lightning_module import LightningModule
    from transformertts_amd.workload import model_config
    cfg = model_config("tiny")
    config = {"model": dict(cfg, device="cpu"), "loss": {"stop_weight": 8.0},
              "training": {"num_epochs": 300, "teacher_forcing_mode": "linear", "warmup_steps": 4000}}
    s = ops.seeds
    saved = (s.base, s.counter, s.explicit, s._derived_from)
    try:
        s.follow_torch()
        draws = []
        for seed in (5, 5, 6):
            torch.manual_seed(seed)
            LightningModule(config)
            s.ensure_seeded()
            draws.append([s.next() for _ in range(3)])
            s.ensure_seeded()                          # a later step of the same module continues the stream
            assert s.counter == 3
        assert draws[0] == draws[1] and draws[0] != draws[2]
        LightningModule(config)                        # a second module mid-run, no re-seed: the stream goes on
        s.ensure_seeded()
        assert s.counter == 3 and s.next() not in draws[2]
        s.counter = 3
        torch.random.manual_seed(6)                    # the other public spelling is counted too
        s.ensure_seeded()
        assert s.counter == 0 and [s.next() for _ in range(3)] == draws[2]
        s.manual_seed(99)
        a = [s.next() for _ in range(2)]
        torch.manual_seed(5)
        LightningModule(config)
        s.ensure_seeded()                              # explicit: neither torch's seed nor a new module moves it
        assert s.counter == 2
        s.manual_seed(99)
        assert [s.next() for _ in range(2)] == a
    finally:
        s.base, s.counter, s.explicit, s._derived_from = saved


def test_mask_arguments_are_read_as_torch_reads_them():
    """transformertts_amd/model/layers.py: which mask tensors become lengths / the causal flag (the kernels' forms) and which
    stay tensors (reference model/layers.py:29-74 hands them to torch's MultiheadAttention)"""
    from transformertts_amd.model import layers as L
    B, T = 3, 9
    lens = torch.tensor([9, 4, 0])
    prefix = torch.arange(T)[None, :] >= lens[:, None]
    got, dead = L._resolve_kpm(prefix, B, T, "cpu")
    assert dead is None and torch.equal(got, lens)
    got, dead = L._resolve_kpm(torch.zeros(B, T).masked_fill(prefix, float("-inf")), B, T, "cpu")     # float form of the same mask
    assert dead is None and torch.equal(got, lens)
    holes = prefix.clone()
    holes[0, 3] = True
    got, dead = L._resolve_kpm(holes, B, T, "cpu")
    assert torch.equal(dead, holes) and got.tolist() == [8, 4, 0]
    with pytest.raises(ValueError):
        L._lens_from_kpm(holes, B, T, "cpu")
    with pytest.raises(ValueError):
        L._resolve_kpm(prefix[:, :5], B, T, "cpu")
    assert L._resolve_kpm(None, B, T, "cpu")[0].tolist() == [T] * B
    causal = torch.triu(torch.ones(T, T, dtype=torch.bool), 1)
    assert L._is_causal_mask(causal, T, T)
    assert L._is_causal_mask(torch.nn.Transformer.generate_square_subsequent_mask(T), T, T)
    assert not L._is_causal_mask(~causal, T, T)
    assert not L._is_causal_mask(torch.nn.Transformer.generate_square_subsequent_mask(T) + torch.eye(T), T, T)
    assert not L._is_causal_mask(causal[:, :5], T, 5)
    a = L._additive_mask(causal, B, 2, T, T)
    assert a.shape == (1, 1, T, T) and a[0, 0, 0, 1] == torch.finfo(torch.float32).min and a[0, 0, 1, 0] == 0
    f = torch.randn(B * 2, T, T)
    assert torch.equal(L._additive_mask(f, B, 2, T, T), f.reshape(B, 2, T, T))
    with pytest.raises(ValueError):
        L._additive_mask(torch.zeros(T + 1, T), B, 2, T, T)
    # non-finite float masks would reach the softmax: refused like a bad float key-padding mask
    for bad in (float("nan"), float("inf")):
        g = f.clone()
        g[0, 0, 0] = bad
        with pytest.raises(ValueError):
            L._additive_mask(g, B, 2, T, T)
    assert torch.isfinite(L._additive_mask(f.masked_fill(f > 1, float("-inf")), B, 2, T, T)).all()
    # lengths AND a key-padding mask: the mask must be the prefix mask of those lengths, or its holes would be lost silently
    got, dead = L._lens_and_kpm(lens, prefix, B, T, "cpu", "x")
    assert dead is None and torch.equal(got, lens)
    with pytest.raises(ValueError):
        L._lens_and_kpm(lens, holes, B, T, "cpu", "x")
    with pytest.raises(ValueError):
        L._lens_and_kpm(torch.tensor([9, 5, 0]), prefix, B, T, "cpu", "x")
    got, dead = L._lens_and_kpm(None, holes, B, T, "cpu", "x")
    assert torch.equal(dead, holes)
