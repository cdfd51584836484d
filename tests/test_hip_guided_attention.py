"""Guided attention loss on the alignment maps (csrc/guided.hip; ops.GuidedAttentionFn; transformertts_amd.loss.GuidedAttentionLoss)
and what it takes to train with it: the loss value and its gradient against an fp64 restatement, head and layer selection,
repeatability; the model's parameter gradients under `total + 0.5 guided` and under `guided` alone against the fp64 oracle
(`TransformerTTS.forward(..., alignments_grad=True)`); `LightningModule.training_step` with config['training']['guided_attention']
eagerly and as a captured graph, and without the key."""
import contextlib
import os

import pytest
import torch

from conftest import rel_l2
from test_hip_dropout_parity import REPORT_DIR
from test_hip_model import FLIP_FREE_GATE, GATE, _build
from test_hip_ops import TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _prior64(plens, mlens, Tm, Tp, sigma):
    """W (B, Tm, Tp) fp64: 1 - exp(-(n / N_b - t / T_b)^2 / (2 sigma^2)) inside each utterance's (T_b, N_b) rectangle, 0 outside"""
    t = torch.arange(Tm, dtype=torch.float64)[None, :, None]
    n = torch.arange(Tp, dtype=torch.float64)[None, None, :]
    T = mlens.double()[:, None, None]
    N = plens.double()[:, None, None]
    W = -torch.expm1(-(n / N.clamp_min(1) - t / T.clamp_min(1)) ** 2 / (2 * sigma ** 2))
    return W * ((t < T) & (n < N))


def _guided64(maps, plens, mlens, sigma, heads=None):
    """the loss restated in fp64: sum over the maps (and the selected heads) of A o W / (n_selected sum_b T_b N_b)"""
    B, H, Tm, Tp = maps[0].shape
    W = _prior64(plens, mlens, Tm, Tp, sigma)
    hs = list(range(H)) if heads is None else list(heads)
    tot = sum((m.double()[:, hs] * W[:, None]).sum() for m in maps)
    return tot / (len(maps) * len(hs) * (plens.clamp(max=Tp) * mlens.clamp(max=Tm)).sum().double())


def _maps(L, B, H, Tm, Tp, plens, mlens, seed):
    """random row-stochastic maps with zeros past the lengths (rows past T_b too)"""
    g = torch.Generator().manual_seed(seed)
    live = (torch.arange(Tp)[None, :] < plens[:, None])[:, None, None, :]
    rows = (torch.arange(Tm)[None, :] < mlens[:, None])[:, None, :, None]
    out = []
    for _ in range(L):
        a = torch.rand(B, H, Tm, Tp, generator=g) * live
        out.append((a / a.sum(-1, keepdim=True).clamp_min(1e-30) * rows).float())
    return out


# B = 4, ragged, with T_b = 1 and N_b = 1; Tp = 13 is no multiple of 4 (the gradient's rows are padded to 16)
PLENS, MLENS = torch.tensor([13, 7, 1, 10]), torch.tensor([37, 1, 20, 29])
SHAPE = dict(L=3, B=4, H=4, Tm=37, Tp=13)


def _run(heads=None, layers=None, sigma=0.4, seed=5, g_up=None):
    """-> (loss on the CPU, [dA per map on the CPU], maps on the CPU)"""
    from transformertts_amd.loss import GuidedAttentionLoss
    maps = _maps(**SHAPE, plens=PLENS, mlens=MLENS, seed=seed)
    dmaps = [m.to(DEV).requires_grad_() for m in maps]
    loss = GuidedAttentionLoss(sigma, heads, layers)(dmaps, PLENS.to(DEV), MLENS.to(DEV))
    loss.backward(None if g_up is None else torch.tensor(g_up, device=DEV))
    torch.cuda.synchronize()
    return loss.detach().cpu(), [None if m.grad is None else m.grad.cpu() for m in dmaps], maps


@pytest.mark.parametrize("sigma", [0.4, 0.05])
def test_guided_loss_value_vs_fp64(sigma):
    loss, _, maps = _run(sigma=sigma)
    ref = float(_guided64(maps, PLENS, MLENS, sigma))
    print(f"guided sigma={sigma}: hip {float(loss):.9f} fp64 {ref:.9f}")
    assert ref > 0 and abs(float(loss) - ref) < 2e-6 * max(1.0, abs(ref))


def test_guided_gradient_vs_fp64_with_exact_zeros_in_the_padding():
    sigma, g_up = 0.4, 0.37
    _, grads, maps = _run(sigma=sigma, g_up=g_up)
    B, H, Tm, Tp = maps[0].shape
    ref = (g_up * _prior64(PLENS, MLENS, Tm, Tp, sigma) / (len(maps) * H * (PLENS * MLENS).sum().double()))[:, None].expand(B, H, Tm, Tp)
    pad = (ref == 0)
    lines = []
    for i, g in enumerate(grads):
        e = rel_l2(g, ref)
        lines.append(f"dA map {i}: {e:.3e} (gate {TOL:g})")
        assert e < TOL, lines
        assert float(g[pad].abs().sum()) == 0.0
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(f"{REPORT_DIR}/guided_attention_grad.txt", "w") as f:
        f.write("\n".join(lines) + "\n")
    # ONE tensor serves every map and, expanded, every head; its rows are 16-byte quads
    from transformertts_amd import ops
    dmaps = [m.to(DEV).requires_grad_() for m in maps]
    loss = ops.GuidedAttentionFn.apply(PLENS.to(DEV), MLENS.to(DEV), sigma, 0, *dmaps)
    got = torch.autograd.grad(loss, dmaps)
    assert len({g.data_ptr() for g in got}) == 1 and got[0].stride() == (Tm * 16, 0, 16, 1)
    assert ops._dattn_in_place(got[0], Tp)


def test_guided_head_and_layer_selection():
    sigma = 0.3
    loss, grads, maps = _run(heads=[2, 0], layers=[2, 0], sigma=sigma)
    ref = float(_guided64([maps[0], maps[2]], PLENS, MLENS, sigma, heads=[0, 2]))
    assert abs(float(loss) - ref) < 2e-6 * max(1.0, abs(ref))
    assert grads[1] is None
    B, H, Tm, Tp = maps[0].shape
    W = _prior64(PLENS, MLENS, Tm, Tp, sigma) / (2 * 2 * (PLENS * MLENS).sum().double())
    for g in (grads[0], grads[2]):
        assert float(g[:, [1, 3]].abs().sum()) == 0.0                # unselected heads: zero planes
        for h in (0, 2):
            assert rel_l2(g[:, h], W) < TOL
    one, _, _ = _run(heads=[3], layers=[1], sigma=sigma)
    ref = float(_guided64([maps[1]], PLENS, MLENS, sigma, heads=[3]))
    assert abs(float(one) - ref) < 2e-6 * max(1.0, abs(ref))
    from transformertts_amd.loss import GuidedAttentionLoss
    dmaps = [m.to(DEV) for m in maps]
    with pytest.raises(ValueError, match="head 4 of 4 heads"):
        GuidedAttentionLoss(heads=[4])(dmaps, PLENS.to(DEV), MLENS.to(DEV))
    with pytest.raises(ValueError, match="layer 3 of 3 alignment maps"):
        GuidedAttentionLoss(layers=[3])(dmaps, PLENS.to(DEV), MLENS.to(DEV))
    with pytest.raises(ValueError, match="no alignment maps"):
        GuidedAttentionLoss()([None, None], PLENS.to(DEV), MLENS.to(DEV))


def test_guided_loss_repeats_bitwise():
    a, ga, _ = _run(heads=[1, 2])
    b, gb, _ = _run(heads=[1, 2])
    assert torch.equal(a, b) and all(torch.equal(x, y) for x, y in zip(ga, gb))


# ============================================================================================ the model
def _oracle_gated_grads(cfg, w_seed, batch, gates, dtype=torch.float64, total_w=1.0, guided_w=0.5, sigma=0.4):
    """the protocol of tests/test_hip_model.py::_oracle_gated_grads -- parameter gradients of the oracle evaluated in `dtype` with
    its ReLUs replaced by the given 0/1 gates, dropout off -- under the loss total_w * total + guided_w * guided, the guided term
    restated in `dtype` on ref['alignments']"""
    from oracle import fill_state, oracle_forward, oracle_loss, relu_gates
    sd = fill_state(cfg, w_seed)
    for k in list(sd):
        if sd[k].is_floating_point():
            sd[k] = sd[k].to(dtype)
            if "running" not in k and k != "pe.pe":
                sd[k].requires_grad_(True)
    with relu_gates(gates=[g.to(dtype) for g in gates]):
        ref = oracle_forward(sd, cfg, batch["phoneme"], batch["melspec"].to(dtype), batch["phoneme_lens"], batch["melspec_lens"],
                             training=True, dropout=False)
    loss = oracle_loss(ref, batch["melspec"].to(dtype), batch["melspec_lens"])
    guided = _guided64(ref["alignments"], batch["phoneme_lens"], batch["melspec_lens"], sigma).to(dtype)
    (total_w * loss["total"] + guided_w * guided).backward()
    return {k: v.grad for k, v in sd.items() if v.requires_grad}, loss, guided


def _model_grads(cfg_name, total_w, guided_w):
    """HIP gradients of total_w * total + guided_w * guided (alignments_grad=True) and the fp64 / stock-fp32 oracles under the HIP
    path's ReLU gates -> (model, hip loss pieces, exact grads, stock-fp32 grads maker, exact guided)"""
    from oracle import synth_batch
    from transformertts_amd import ops
    from transformertts_amd.loss import GuidedAttentionLoss, TransformerTTSLoss
    w_seed, b_seed = (11, 21) if cfg_name == "tiny" else (16, 26)
    cfg, m = _build(cfg_name, w_seed)
    batch = synth_batch(3, 12, 40, cfg["n_mels"], cfg["n_phon"], ragged=True, seed=b_seed)
    args = [batch[k].to(DEV) for k in ("phoneme", "melspec", "phoneme_lens", "melspec_lens")]
    m.train()
    gates = []
    ops._relu_observer = lambda y: gates.append((y.detach() > 0).cpu())
    try:
        out = m(*args, need_alignments=True, alignments_grad=True)
    finally:
        ops._relu_observer = None
    assert all(a.requires_grad for a in out["alignments"])
    total = TransformerTTSLoss(8.0).to(DEV)(out, args[1], args[3])["total"]
    guided = GuidedAttentionLoss(0.4)(out["alignments"], args[2], args[3])
    (guided_w * guided if total_w == 0 else total_w * total + guided_w * guided).backward()
    torch.cuda.synchronize()
    exact, rloss, rguided = _oracle_gated_grads(cfg, w_seed, batch, gates, total_w=total_w, guided_w=guided_w)
    stock = lambda: _oracle_gated_grads(cfg, w_seed, batch, gates, dtype=torch.float32, total_w=total_w, guided_w=guided_w)[0]
    assert abs(float(guided.detach()) - float(rguided.detach())) < 2e-6 * max(1.0, abs(float(rguided.detach())))
    assert abs(float(total.detach()) - float(rloss["total"].detach())) < 1e-5 * abs(float(rloss["total"].detach()))
    return m, exact, stock


def _compare(m, exact, stock, report):
    """every parameter with a gradient at FLIP_FREE_GATE; one above it is held to twice what stock fp32 torch makes under the same
    gates and never above 1e-4 (the rule of tests/test_hip_model.py::test_forward_backward_vs_oracle); -> names compared"""
    errs, seen = {}, []
    for name, p in m.named_parameters():
        rg = exact[name]
        if rg is None or rg.norm().item() < 1e-7 * max(1.0, p.detach().norm().item()):      # analytically zero, or out of reach
            assert p.grad is None or p.grad.abs().max().item() < 1e-4, name
            continue
        assert p.grad is not None, name
        errs[name] = rel_l2(p.grad, rg)
        seen.append(name)
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(f"{REPORT_DIR}/guided_attention_{report}.txt", "w") as f:
        for k, v in sorted(errs.items(), key=lambda kv: -kv[1]):
            f.write(f"{v:.3e} grad/{k}\n")
    print(report, "worst", max(errs.items(), key=lambda kv: kv[1]))
    over = {k: v for k, v in errs.items() if not v < FLIP_FREE_GATE}
    bad = {}
    if over:
        s32 = stock()
        for k, v in over.items():
            e32 = rel_l2(s32[k], exact[k])
            if not (v < 2.0 * e32 and v < GATE):
                bad[k] = (v, e32)
    assert not bad, bad
    return seen


@pytest.mark.parametrize("cfg_name", ["tiny", "micro"])
def test_model_gradients_under_total_plus_guided_vs_oracle(cfg_name):
    """B = 3, Tp = 12, Tm = 40, dropout off, loss = total + 0.5 guided: every parameter gradient against the fp64 oracle under the
    HIP path's ReLU gates with the fp64 guided term on ref['alignments']"""
    m, exact, stock = _model_grads(cfg_name, 1.0, 0.5)
    seen = _compare(m, exact, stock, f"model_{cfg_name}_total_plus_guided")
    assert len(seen) > 0.8 * len(list(m.parameters()))


@pytest.mark.parametrize("cfg_name", ["tiny", "micro"])
def test_model_gradients_under_guided_alone_vs_oracle(cfg_name):
    """the loss is `guided` alone: the maps are all that carries a gradient, and it reaches the decoder's in-projections and the
    encoder -- non-zero there, and equal to the oracle's"""
    m, exact, stock = _model_grads(cfg_name, 0.0, 1.0)
    seen = _compare(m, exact, stock, f"model_{cfg_name}_guided_alone")
    for needle in ("decoder.layers.0.multihead_attn.in_proj_weight", "decoder.layers.0.self_attn.in_proj_weight",
                   "encoder.layers.0.self_attn.in_proj_weight", "encoder.layers.0.linear1.weight"):
        assert needle in seen, needle
        assert float(dict(m.named_parameters())[needle].grad.abs().max()) > 0


def test_alignments_grad_refusal_and_default():
    cfg, m = _build("tiny", 11)
    from oracle import synth_batch
    batch = synth_batch(2, 10, 20, cfg["n_mels"], cfg["n_phon"], ragged=True, seed=3)
    args = [batch[k].to(DEV) for k in ("phoneme", "melspec", "phoneme_lens", "melspec_lens")]
    with pytest.raises(ValueError, match="alignments_grad=True needs need_alignments=True"):
        m(*args, need_alignments=False, alignments_grad=True)
    m.train()
    assert not any(a.requires_grad for a in m(*args)["alignments"])            # without the flag the maps stay detached


# ============================================================================================ the training step
def _setup(guided, w_seed=3, epoch=150):
    from oracle import fill_state
    from transformertts_amd.lightning_module import LightningModule
    from transformertts_amd.workload import model_config
    cfg = model_config("tiny")
    training = {"num_epochs": 300, "teacher_forcing_mode": "linear", "warmup_steps": 50, "sync_loss_every_step": False,
                "fused_clip_norm": 1.0}
    if guided is not None:
        training["guided_attention"] = guided
    lm = LightningModule({"model": dict(cfg, device="cuda"), "loss": {"stop_weight": 8.0}, "training": training}).to("cuda")
    lm.model.load_state_dict(fill_state(cfg, w_seed), strict=True)
    lm.train()
    lm.current_epoch = epoch
    oc = lm.configure_optimizers()
    return cfg, lm, oc["optimizer"], oc["lr_scheduler"]["scheduler"]


def _steps(guided, graph, n, accumulate=1):
    from transformertts_amd.step import TrainStep
    from transformertts_amd.workload import synth_batch
    cfg, lm, opt, sch = _setup(guided)
    batch = {k: v.to("cuda") for k, v in synth_batch(3, 12, 40, cfg["n_mels"], cfg["n_phon"], ragged=True, seed=8).items()}
    ts = TrainStep(lm, opt, sch, batch, graph=graph, seed=77, accumulate=accumulate)
    losses = [ts().detach().clone() for _ in range(n)]
    torch.cuda.synchronize()
    assert ts.graphed == graph
    bn = {k: v.clone() for k, v in lm.model.state_dict().items() if "running" in k or "num_batches" in k}
    return losses, opt.flat_params.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), bn


def _same_runs(a, b):
    for x, y in zip(a[0], b[0]):
        assert torch.isfinite(x) and torch.equal(x, y)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    for k in a[4]:
        assert torch.equal(a[4][k], b[4][k]), k


@pytest.mark.parametrize("accumulate", [1, 2])
def test_guided_training_step_graph_replay_equals_eager_bitwise(accumulate):
    """tiny config, dropout on, scheduled sampling active, guided attention {weight 0.5, sigma 0.4, heads [0]}: 2 eager + 3 replayed
    steps equal 5 eager steps bit for bit (parameters, Adam moments, BatchNorm buffers, per-step losses); the captured step holds
    no host read"""
    ga = {"weight": 0.5, "sigma": 0.4, "heads": [0]}
    n = 5 * accumulate
    eager, graphed = _steps(ga, False, n, accumulate), _steps(ga, True, n, accumulate)
    _same_runs(eager, graphed)
    assert len({float(x) for x in eager[0]}) == n
    # ... and the term is in the loss and in the update
    plain = _steps(None, False, n, accumulate)
    assert not torch.equal(plain[1], eager[1]) and float(eager[0][0]) > float(plain[0][0])


def test_training_step_without_the_key_is_todays_step():
    """config['training'] without `guided_attention` (or with None): the step's loss and gradients are bit-identical to a forward
    with need_alignments=False and the flags off, written out here"""
    from transformertts_amd import ops
    from transformertts_amd.utils.util import apply_teacher_forcing, prepare_batch
    from transformertts_amd.workload import synth_batch
    runs = []
    for mode in ("absent", "none", "by_hand"):
        cfg, lm, _, _ = _setup({"absent": None, "none": None, "by_hand": None}[mode])
        if mode == "none":
            lm.config["training"]["guided_attention"] = None
        assert lm.guided is None
        batch = {k: v.to("cuda") for k, v in synth_batch(3, 12, 40, cfg["n_mels"], cfg["n_phon"], ragged=True, seed=8).items()}
        torch.manual_seed(5)
        ops.seeds.manual_seed(1234)
        try:
            if mode != "by_hand":
                loss = lm.training_step(batch, 0)
            else:
                phoneme, melspec, plens, mlens = prepare_batch(batch, lm.device)
                mem_g, mem_n = lm.model.encode_twin(phoneme, plens) if lm.model.twin_encode_ok(phoneme) else (None, None)
                twin = ops.PostnetTwin() if lm.model.twin_postnet_ok(melspec) else None
                with torch.no_grad():
                    pred = lm.model(phoneme, melspec, plens, mlens, need_alignments=False, need_stop=False, memory=mem_n,
                                    postnet_twin=twin)["pred_melspec"]
                mixed = apply_teacher_forcing(pred, melspec, mlens, lm.teacher_forcing_ratio(), lm.device)
                out = lm.model(phoneme, mixed, plens, mlens, need_alignments=False, alignments_grad=False, memory=mem_g,
                               postnet_twin=twin)
                loss = lm.criterion(out, melspec, mlens)["total"]
            loss.backward()
        finally:
            ops.seeds.follow_torch()
        torch.cuda.synchronize()
        runs.append((loss.detach().clone(), {n: p.grad.clone() for n, p in lm.model.named_parameters() if p.grad is not None}))
    for other in runs[1:]:
        assert torch.equal(runs[0][0], other[0])
        assert runs[0][1].keys() == other[1].keys()
        for k in runs[0][1]:
            assert torch.equal(runs[0][1][k], other[1][k]), k
