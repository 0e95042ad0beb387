"""LightweightMobileNet on the HIP path: packed training, LocalTrainer, eval-mode forward, a
RankRound round (eager == graph / program replay, FedAvg, update-level DP) against the CPU
restatement of the reference (tests/mobilenet_ref.py, pinned by test_mobilenet_ref_cpu.py).

Criterion: check_params / check_loss of tests/test_train_gpu.py — the HIP result must be as
close to an fp64 run REPLAYING the HIP run's ReLU masks as the fp32 CPU run is, times 4 plus
a floor; under Adam at most 0.1 % of a tensor's elements (at least 2) may sit outside
1e-2 lr, bounded by 2 lr steps.  That cap is a condition on the reference too: the fp32 CPU
run, judged against the fp64 run replaying ITS OWN masks, must stay inside it.  At the
constructor's BatchNorm values (weight 1, bias 0) it does not, for any seed tried (init /
data 21/300, 22/310, 23/320, 24/330: 3-6 outliers in the 32..128-element bn weights against
2 allowed): relu(w * xhat) = w * relu(xhat) there, and the depthwise conv + BatchNorm that
follow are per-channel and scale-invariant, so the gradient of those BN weights is
analytically zero and Adam turns its rounding noise into O(lr) updates — the situation
check_params already exempts for conv biases in front of a BatchNorm.  The packed parity
cases therefore start from seeded non-degenerate BatchNorm affines (weight U(0.5, 1.5), bias
0.2 N(0, 1), generator seed INIT_SEED + 1000) on both sides; with them seeds 21 / 300 keep
the fp32 CPU run inside the cap for SGD, Adam and AdamW over both steps of every client
(checked on the CPU).  The width-1.0, LocalTrainer and RankRound cases (SGD) keep the
constructor's values.
"""
import math

import numpy as np
import pytest
import torch

import mobilenet_ref as mr
from fedhip._lib import FedHipError
from fedhip.engine import DPSGDConfig, PackedTrainer
from fedhip.round import DPConfig, RankRound
from oracle import fedavg_ref, privacy_ref
from src.shared import models_pytorch as hm
from src.shared.training import LocalTrainer
from test_train_gpu import check_loss, check_params

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
INIT_SEED, DATA_SEED = 21, 300


def make_batch(n, seed, cin=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, cin, 32, 32, generator=g), torch.randint(0, 10, (n,), generator=g)


def hip_model(width, seed=INIT_SEED):
    torch.manual_seed(seed)
    return hm.ModelFactory.create_model("lightweight_mobilenet", width_multiplier=width)


def masks_of(eng, slots):
    """Per slot, the 13 ReLU masks of the step just run."""
    bufs = [(b[:slots] > 0).cpu() for b in eng.net.relu_output_buffers()]
    assert len(bufs) == 13
    return [[b[s] for b in bufs] for s in range(slots)]


def perturb_bn(ref, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if ".bn" in n or n.startswith("bn"):
                if n.endswith("weight"):
                    p.copy_(0.5 + torch.rand(p.shape, generator=g))
                else:
                    p.copy_(0.2 * torch.randn(p.shape, generator=g))


def _packed_parity(width, sizes, B, opt, lr, bn_seed=None):
    model = hip_model(width)
    ref0 = mr.init_model(INIT_SEED, width)
    if bn_seed is not None:
        perturb_bn(ref0, bn_seed)
        model.set_model_weights({k: v.detach().clone() for k, v in ref0.named_parameters()})
    init = {k: p.detach().clone() for k, p in ref0.named_parameters()}
    for n, p in model.named_parameters():
        assert torch.equal(p.detach(), init[n]), n
    datas = [make_batch(s, DATA_SEED + i) for i, s in enumerate(sizes)]
    eng = PackedTrainer(model.to(DEV), capacity=len(sizes), batch=B, device=DEV)
    for k in range(len(sizes)):
        eng.load_module_state(k, model)
    plan = eng.make_plan(sizes, 1, generator=torch.Generator().manual_seed(5))
    data = torch.cat([d[0] for d in datas]).to(DEV)
    labels = torch.cat([d[1] for d in datas]).to(DEV)
    offs = np.cumsum([0] + sizes[:-1]).tolist()
    snaps, rows = [], []

    def on_step(e, n):
        snaps.append(masks_of(e, n))
        rows.append([e.weights_dict(k) for k in range(n)])
    eng.on_step = on_step
    metrics = eng.run_round(data, labels, offs, plan, optimizer_type=opt, lr=lr)
    torch.cuda.synchronize()
    # the same round without a step hook: every step after the first is a HIP-graph replay
    # (PackedTrainer's and LocalTrainer's default) — the same bits as the eager steps
    rep = PackedTrainer(model, capacity=len(sizes), batch=B, device=DEV)
    for k in range(len(sizes)):
        rep.load_module_state(k, model)
    m2 = rep.run_round(data, labels, offs, plan, optimizer_type=opt, lr=lr)
    torch.cuda.synchronize()
    if plan["G"] > 1:
        assert rep.launch_mode == "graph" and rep._graphs
        assert all(p is None for _, p in rep._graphs.values())
    assert torch.equal(rep.params.view(torch.int32), eng.params.view(torch.int32))
    assert torch.equal(rep.bufs.view(torch.int32), eng.bufs.view(torch.int32))
    assert [m.loss for m in m2] == [m.loss for m in metrics]
    rep.release_graphs()
    for k, s in enumerate(sizes):
        ref, ref64 = ref0.clone(), ref0.double()
        optr, opt64 = mr.make_optimizer(ref, opt, lr), mr.make_optimizer(ref64, opt, lr)
        st = math.ceil(s / B)
        running, r64, correct = 0.0, 0.0, 0
        for g in range(st):
            idx = plan["index"][g, k, :plan["counts"][g, k]]
            m = idx.numel()
            xb, yb = datas[k][0][idx], datas[k][1][idx]
            li, c, _, _ = mr.train_step(ref, optr, xb, yb)
            l64, _, _, _ = mr.train_step(ref64, opt64, xb.double(), yb,
                                         relus=[r[:m] for r in snaps[g][k]])
            running, r64, correct = running + li, r64 + l64, correct + c
            # one-step and two-step parity
            check_params(rows[g][k], ref, ref64, init, g + 1, lr, opt)
        check_loss(metrics[k].loss, running / st, r64 / st)
        assert abs(metrics[k].accuracy - correct / s) <= 1.0 / s + 1e-12
        assert metrics[k].samples_processed == s


@pytest.mark.parametrize("opt,lr", [("sgd", 0.01), ("adam", 1e-3), ("adamw", 1e-3)])
def test_packed_training_parity(opt, lr):
    """Width 0.5, 3 clients, batch 8, two steps each, the last client's last batch ragged."""
    _packed_parity(0.5, [16, 16, 11], 8, opt, lr, bn_seed=INIT_SEED + 1000)


def test_packed_training_parity_width_1():
    """Width 1.0 (512-feature classifier: the unfused head), 1 client, batch 4, SGD."""
    _packed_parity(1.0, [8], 4, "sgd", 0.01)


def test_local_trainer_matches_helper():
    n, bs, lr = 24, 8, 0.01
    torch.manual_seed(INIT_SEED)
    model = hm.ModelFactory.get_lightweight_model()
    ref0 = mr.init_model(INIT_SEED, 0.5)
    init = {k: p.detach().clone() for k, p in ref0.named_parameters()}
    x, y = make_batch(n, DATA_SEED + 7)
    batches = [(x[i:i + bs], y[i:i + bs]) for i in range(0, n, bs)]
    ref = ref0.clone()
    mref = mr.train_epochs(ref, batches, 1, lr, "sgd")
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(x, y), batch_size=bs,
                                         shuffle=False)
    tr = LocalTrainer(model, device=DEV)
    snaps = []
    tr._engine(bs).on_step = lambda e, k: snaps.append(masks_of(e, 1)[0])
    m = tr.train_local_model(loader, epochs=1, learning_rate=lr, optimizer_type="sgd",
                             save_checkpoints=False)
    ref64 = ref0.double()
    m64 = mr.train_epochs(ref64, [(a.double(), b) for a, b in batches], 1, lr, "sgd",
                          relus=[[r[:a.shape[0]] for r in sn] for sn, (a, _) in zip(snaps, batches)])
    assert m.samples_processed == n and m.epochs_completed == 1
    check_loss(m.loss, mref["loss"], m64["loss"])
    assert abs(m.accuracy - mref["accuracy"]) <= 1.0 / n + 1e-12
    check_params(dict(model.named_parameters()), ref, ref64, init, len(batches), lr, "sgd")
    sd = model.state_dict()
    for k, v in ref.buffers.items():
        if "running" in k:
            d = (sd[k].cpu().double() - v.double()).abs().max().item()
            assert d <= 1e-4 * max(1.0, v.abs().max().item()), k


@pytest.mark.parametrize("width,cin", [(0.5, 3), (1.0, 1)])
def test_eval_forward_matches_helper(width, cin):
    """Eval-mode model(x): logits within the fp32 tolerance of test_eval_surface_gpu.py;
    predictions equal wherever the helper's top-2 margin is clear of it."""
    torch.manual_seed(3)
    model = hm.LightweightMobileNet(num_classes=10, width_multiplier=width, input_channels=cin)
    ref = mr.init_model(3, width, input_channels=cin)
    g = torch.Generator().manual_seed(4)
    # non-trivial running statistics and affine
    for k, b in ref.buffers.items():
        if k.endswith("running_mean"):
            b.copy_(0.1 * torch.randn(b.shape, generator=g))
        elif k.endswith("running_var"):
            b.copy_(0.5 + torch.rand(b.shape, generator=g))
    model.load_state_dict({**{k: v.detach() for k, v in ref.params.items()}, **ref.buffers})
    x, _ = make_batch(37, 9, cin)
    logits = mr.eval_logits(ref, x)
    model = model.to(DEV).eval()
    with torch.no_grad():
        got = model(x.to(DEV)).cpu()
    tol = 2e-4 * float(logits.abs().max()) + 1e-5
    assert (got - logits).abs().max().item() <= tol
    top2 = logits.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 4 * tol
    assert bool(clear.any())
    assert torch.equal(got.argmax(1)[clear], logits.argmax(1)[clear])


def _split(row, layout):
    return [row[o:o + int(np.prod(s))].reshape(s) for o, s in zip(layout.offsets, layout.shapes)]


def test_rank_round_replay_fedavg_dp():
    """One RankRound round of 4 clients with unequal step counts: the graph / program replay
    reproduces the eager round's trained rows bit for bit; FedAvg of the parameters and BN
    statistics is bit-exact against oracle.fedavg_ref on the GPU-trained rows; update-level DP
    with injected noise matches oracle.privacy_ref."""
    sizes, B, E, eps = [40, 24, 17, 9], 8, 1, 2.0
    model = hip_model(0.5)
    rr = RankRound(model.to(DEV), sizes, list(range(4)), epochs=E, batch=B, device=DEV,
                   shuffle_seed=123, dp_seed=9, dp=DPConfig(epsilon=eps))
    tr = rr.trainer
    L, S, P = tr.layout, len(rr.slots), rr.P
    g = torch.Generator().manual_seed(77)
    datas = {k: make_batch(n, 50 + k) for k, n in enumerate(sizes)}
    data = torch.cat([datas[k][0] for k in rr.slots]).to(DEV)
    labels = torch.cat([datas[k][1] for k in rr.slots]).to(DEV)
    offs = np.cumsum([0] + [sizes[k] for k in rr.slots][:-1]).tolist()
    G0 = rr.global_flat.clone()
    noise = 1e-3 * torch.randn(S, P, generator=g)
    rr.dp_noise = noise.to(DEV)
    trained = {}
    rr.on_trained = lambda params, s: trained.__setitem__("rows", params[:s, :P].clone())
    for ln in tr.lanes:  # a step hook keeps every step eager
        ln.on_step = lambda e, n: None
    metrics = rr.run(data, labels, offs, "sgd", 0.01, seed=0)
    torch.cuda.synchronize()
    R = trained["rows"].cpu().numpy()
    G1 = rr.global_flat.cpu().numpy().copy()
    GB1 = rr.global_bufs[:L.Q].cpu().numpy().copy()
    final = tr.params[:S, :P].cpu().numpy()
    bufs = tr.bufs[:S, :L.Q].cpu().numpy()
    assert [m.samples_processed for m in metrics] == [E * sizes[k] for k in rr.slots]
    assert np.isfinite(R).all() and not np.array_equal(R[0], G0.cpu().numpy())

    for ln in tr.lanes:
        ln.on_step = None
    for mode in ("graph", "program"):  # every step after a lane's first is replayed
        for ln in tr.lanes:
            ln.release_graphs()  # the captured steps are cached without their mode
            ln.launch_mode = mode
        for rep in range(2):  # captured in the first round, replayed in both
            rr.set_global(G0)
            rr.run(data, labels, offs, "sgd", 0.01, seed=0)
            torch.cuda.synchronize()
            Rt = trained["rows"].cpu().numpy()
            bad = [i for i in range(S) if not np.array_equal(Rt[i].view(np.uint32),
                                                             R[i].view(np.uint32))]
            assert not bad, f"{mode} replay {rep}: rows of slots {bad} differ from the eager round"
        progs = [p for ln in tr.lanes for _, p in ln._graphs.values()]
        assert progs and all((p is not None) == (mode == "program") for p in progs), mode

    gparts = _split(G0.cpu().numpy(), L)
    for i in range(S):
        out, _, _, _ = privacy_ref.apply_update_dp(_split(R[i], L), gparts, 1.0, eps, 1e-5,
                                                   _split(noise[i].numpy(), L))
        e = np.concatenate([o.reshape(-1) for o in out])
        d = np.abs(final[i].astype(np.float64) - e)
        assert d.max() <= 4 * np.finfo(np.float32).eps * max(1.0, np.abs(e).max()), i
    w = fedavg_ref.calculate_sample_weights([E * n for n in sizes])
    glob = fedavg_ref.weighted_average([final[rr.slot_of[k]] for k in range(4)], w)
    assert np.array_equal(G1.view(np.uint32), glob.view(np.uint32))
    gb = fedavg_ref.weighted_average([bufs[rr.slot_of[k]] for k in range(4)], w)
    assert np.array_equal(GB1.view(np.uint32), gb.view(np.uint32))
    # the FedAvg'd model evaluates (GlobalEvaluator, BN statistics averaged)
    xt, yt = make_batch(20, 99)
    ev = rr.evaluate(xt.to(DEV), yt.to(DEV))
    assert ev["total_samples"] == 20 and math.isfinite(ev["loss"])


def test_dpsgd_still_refused():
    model = hip_model(0.5).to(DEV)
    eng = PackedTrainer(model, capacity=1, batch=8, device=DEV, dpsgd=DPSGDConfig(seed=1))
    eng.load_module_state(0, model)
    eng.begin_round("sgd", 0.01)
    x, y = make_batch(8, 1)
    eng.net.x[0].copy_(x)
    eng.net.y[0].copy_(y)
    with pytest.raises(FedHipError, match="BatchNorm"):
        eng.step(1, torch.tensor([8], dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
