"""GPU tests of the inference kernels and the native inference engine
(MI355X).  Run with: pytest tests -m gpu"""
import pytest
import torch
import torch.nn.functional as F

from heterofl_amd import ops as native_ops
from heterofl_amd.ops.fused import (bn_relu_infer, conv_fwd_large,
                                    conv_pack_weight, eval_metrics, fold_bn,
                                    grouped_conv)
from tests.conftest import make_cfg
from tests.test_infer import eval_case, check_eval_case

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason='no GPU')
DEV = 'cuda:0'

# (N, Cin, H, Cout, k, stride, pad)
CONV_SHAPES = [
    (3, 64, 8, 64, 3, 1, 1),       # P=192: tiles cross samples, ragged tail
    (5, 20, 7, 36, 3, 2, 1),       # odd spatial, stride 2, ragged channels
    (2, 3, 32, 64, 3, 1, 1),       # K=27 < BK
    (4, 128, 16, 256, 1, 2, 0),    # 1x1 stride 2
    (2, 4, 32, 4, 3, 1, 1),        # rate-e widths
    (70, 512, 4, 512, 3, 1, 1),    # K=4608, P=1120, many samples per tile
    (2, 256, 4, 1024, 1, 1, 0),    # bottleneck expansion
]
CONV_CASES = [(s, False) for s in CONV_SHAPES] + \
    [(CONV_SHAPES[0], True), (CONV_SHAPES[3], True)]


@needs_gpu
@pytest.mark.parametrize('shape,extras', CONV_CASES)
def test_conv_fwd_large_matches_conv2d(shape, extras):
    """|y - ref| <= 2^-8 |ref| + K 2^-23 A elementwise, A = conv(|x|, |w|):
    bf16 output rounding plus the fp32 accumulation forward error bound.
    The reference runs in fp32 (on the host) on bf16-rounded inputs."""
    N, Cin, H, Cout, k, s, p = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(N, Cin, H, H, generator=g).bfloat16()
    w = (torch.randn(Cout, Cin, k, k, generator=g) * 0.1).bfloat16().float()
    bias = res = None
    ref = F.conv2d(x.float(), w, None, s, p)
    A = F.conv2d(x.float().abs(), w.abs(), None, s, p)
    if extras:
        bias = torch.randn(Cout, generator=g)
        res = torch.randn(ref.shape, generator=g).bfloat16()
        ref = ref + bias.view(1, -1, 1, 1) + res.float()
    packed = conv_pack_weight(w.to(DEV))
    y = conv_fwd_large(x.to(DEV), packed,
                       None if bias is None else bias.to(DEV),
                       None if res is None else res.to(DEV), s, p, Cin, Cout,
                       k)
    torch.cuda.synchronize()
    assert y.dtype == torch.bfloat16 and y.shape == ref.shape
    K = Cin * k * k
    err = (y.float().cpu() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * A
    worst = (err - bound).max().item()
    print('conv_fwd_large', shape, extras, 'max err', err.max().item(),
          'max(err - bound)', worst)
    assert worst <= 0, (shape, worst)


@needs_gpu
@pytest.mark.parametrize('shape', [(3, 5, 7, 7), (2, 64, 32, 32)])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_bn_relu_infer(shape, dtype):
    g = torch.Generator().manual_seed(1)
    C = shape[1]
    x = torch.randn(shape, generator=g).to(dtype)
    w = torch.randn(C, generator=g)
    b = torch.randn(C, generator=g)
    mean = torch.randn(C, generator=g)
    var = torch.rand(C, generator=g) + 0.5
    ref = F.relu(F.batch_norm(x.float(), mean, var, w, b, training=False,
                              eps=1e-5))
    scale, shift = fold_bn(w, b, mean, var, 1e-5)
    y = bn_relu_infer(x.to(DEV), scale.to(DEV), shift.to(DEV))
    assert y.dtype == dtype
    err = (y.float().cpu() - ref).abs()
    if dtype == torch.float32:
        assert err.max().item() <= 1e-5 * ref.abs().max().item()
    else:
        assert ((err - (2.0 ** -8 * ref.abs() + 1e-3)).max().item() <= 0)


@needs_gpu
def test_eval_metrics_device():
    case = eval_case(DEV)
    local, glob = eval_metrics(case['scores'], case['labels'], case['ptr'],
                               case['samples'], case['mask'])
    check_eval_case(local, glob, case)
    # deterministic: a second launch reproduces the sums bit for bit
    local2, glob2 = eval_metrics(case['scores'], case['labels'], case['ptr'],
                                 case['samples'], case['mask'])
    assert torch.equal(local, local2) and torch.equal(glob, glob2)


# ----------------------------------------------------------- NativeInference
def _tracked_model(base_cfg, model_name, data_name, norm='bn'):
    from heterofl_amd.models import make_model
    cfg = make_cfg(base_cfg, '1_4_0.5_iid_fix_a1_{}_1_1'.format(norm),
                   data_name=data_name, model_name=model_name)
    torch.manual_seed(3)
    model = make_model(cfg, model_rate=1, track=True)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(0.2 * torch.randn_like(m.running_mean))
                m.running_var.copy_(0.6 + 0.8 * torch.rand_like(m.running_var))
                m.weight.add_(0.1 * torch.randn_like(m.weight))
                m.bias.add_(0.1 * torch.randn_like(m.bias))
    model = model.to(DEV)
    model.train(False)
    shape = (64, 3, 32, 32) if data_name == 'CIFAR10' else (64, 1, 28, 28)
    x = torch.randn(shape, device=DEV)
    return model, x


def _eager_logits(model, x):
    with torch.no_grad():
        label = torch.zeros(x.size(0), dtype=torch.long, device=x.device)
        return model({'img': x, 'label': label})['score'].float()


def _rel_err(got, ref):
    return ((got - ref).abs().max() / ref.abs().max()).item()


def bf16_bound(model, x, ref):
    """The bf16 error budget of the evaluator is not fixed in advance: it is
    measured on the device as the error of the SAME evaluator routed through
    the existing conv_fwd in bf16 against the fp32 eager logits (normalised
    by max|ref|), and the large-kernel path is allowed 2x that — only the
    summation order differs between the two conv kernels.
    Measured on MI355X (batch 64, this file's models), error / max|ref|:
      resnet18: conv_fwd 1.97e-3 -> bound 3.94e-3; large kernel 2.19e-3
                (every supported conv) / 2.21e-3 (routed)
      conv:     conv_fwd 2.73e-3 -> bound 5.47e-3; large kernel 2.73e-3
      test_levels level a vs stats() (80 samples): conv_fwd 1.62e-2 ->
                bound 3.24e-2; level-a model through the large kernel 1.67e-2"""
    from heterofl_amd.fed.infer import NativeInference
    old = _rel_err(NativeInference(model, torch.bfloat16, large=False)(x),
                   ref)
    return old, 2.0 * old


@needs_gpu
@pytest.mark.parametrize('model_name,data_name', [
    ('resnet18', 'CIFAR10'), ('conv', 'MNIST')])
def test_native_inference_fp32(base_cfg, model_name, data_name):
    from heterofl_amd.fed.infer import NativeInference
    model, x = _tracked_model(base_cfg, model_name, data_name)
    ref = _eager_logits(model, x)
    got = NativeInference(model, torch.float32, large=False)(x)
    assert got.dtype == torch.float32 and got.shape == ref.shape
    assert _rel_err(got, ref) <= 1e-3


@needs_gpu
@pytest.mark.parametrize('model_name,data_name', [
    ('resnet18', 'CIFAR10'), ('conv', 'MNIST')])
def test_native_inference_bf16_large(base_cfg, model_name, data_name):
    # measured values and the resulting bounds: see bf16_bound
    from heterofl_amd.fed.infer import NativeInference
    model, x = _tracked_model(base_cfg, model_name, data_name)
    ref = _eager_logits(model, x)
    old, bound = bf16_bound(model, x, ref)
    for large in ('all', True):
        new = _rel_err(NativeInference(model, torch.bfloat16, large=large)(x),
                       ref)
        print('bf16 evaluator', model_name, 'large =', large,
              'old conv_fwd err', old, 'bound', bound, 'large err', new)
        assert new <= bound, (model_name, large, new, bound)


@needs_gpu
def test_native_inference_gn(base_cfg):
    """gn has no running statistics: the existing gn_relu_fwd is reused."""
    from heterofl_amd.fed.infer import NativeInference
    model, x = _tracked_model(base_cfg, 'resnet18', 'CIFAR10', norm='gn')
    ref = _eager_logits(model, x)
    got = NativeInference(model, torch.float32, large=False)(x)
    assert _rel_err(got, ref) <= 1e-3


# -------------------------------------------------------------- test_levels
@needs_gpu
def test_levels_gpu(base_cfg):
    from heterofl_amd.data import fetch_dataset, split_dataset
    from heterofl_amd.fed import FedRunner
    from heterofl_amd.fed.infer import NativeInference
    from heterofl_amd.models import make_model
    from heterofl_amd.utils import process_dataset, make_optimizer
    cfg = make_cfg(base_cfg, '1_4_0.5_iid_fix_a1-c1-e1_bn_1_1',
                   data_name='CIFAR10', model_name='resnet18')
    cfg['device'] = DEV
    cfg['engine'] = 'batched'
    cfg['compute_dtype'] = 'bfloat16'
    torch.manual_seed(0)
    ds = fetch_dataset('CIFAR10', synthetic=True, synthetic_size=80)
    process_dataset(ds, cfg)
    data_split, label_split = split_dataset(ds, 4, 'iid', cfg['classes_size'])
    model = make_model(cfg).to(DEV)
    runner = FedRunner(cfg, ds, data_split, label_split, model,
                       make_optimizer(model, cfg['lr'], cfg))
    # same seed before both passes: the train-time crops/flips then agree
    torch.manual_seed(11)
    stats_model = runner.stats()
    torch.manual_seed(11)
    levels = runner.test_levels(1)
    assert sorted(levels) == [0.0625, 0.25, 1.0]
    for lv in levels.values():
        assert len(lv) == 4
        assert all(torch.isfinite(torch.tensor(v)) for v in lv.values())
    img, _, aug = runner._stage_eval()
    x = aug(img, train=False)
    ref = _eager_logits(stats_model, x)
    old, bound = bf16_bound(stats_model, x, ref)
    got = NativeInference(runner.level_models[1.0])(x)
    err = _rel_err(got, ref)
    print('level a vs stats(): err', err, 'old', old, 'bound', bound)
    assert err <= bound


# ------------------------------------------------------------- grouped_conv
@needs_gpu
def test_grouped_conv_large_route():
    ext = native_ops.require_native()
    g = torch.Generator().manual_seed(2)
    from heterofl_amd.ops.fused import large_conv_route
    assert large_conv_route(64, 64, 16, 16, 128, 3, 1, 1)
    x = torch.randn(64, 64, 16, 16, generator=g).bfloat16().to(DEV)
    w = torch.nn.Parameter((torch.randn(128, 64, 3, 3, generator=g) * 0.1)
                           .to(DEV))
    res = torch.randn(64, 128, 16, 16, generator=g).bfloat16().to(DEV)
    none = torch.Tensor()
    old = ext.conv_fwd(x, w.detach(), none, res, 1, 1, 1, 0)
    direct = conv_fwd_large(x, conv_pack_weight(w.detach()), None, res, 1, 1,
                            64, 128, 3)
    prev = native_ops.set_large_conv(True)
    try:
        with torch.no_grad():
            y = grouped_conv(x, w, None, 1, 1, 1, residual=res)
        assert torch.equal(y, direct)
        # a gradient is required: the training kernel family runs
        yg = grouped_conv(x, w, None, 1, 1, 1, residual=res)
        assert yg.grad_fn is not None
        assert torch.equal(yg.detach(), old)
    finally:
        native_ops.set_large_conv(prev)
    # switch off: nothing changes
    with torch.no_grad():
        assert torch.equal(grouped_conv(x, w, None, 1, 1, 1, residual=res),
                           old)


# --------------------------------------------------------- HETEROFL_NATIVE_EVAL
@needs_gpu
def test_native_eval_knob(base_cfg, monkeypatch):
    """runner.test() under HETEROFL_NATIVE_EVAL=1 logs exactly the means of
    the eval_metrics sums over the NativeInference logits.  Against the
    eager evaluation the losses obey |dCE| <= 2 max|dlogit| (cross-entropy
    is 1-Lipschitz in the sup norm in both the log-sum-exp and the picked
    logit; the label mask zeroes the same entries on both sides)."""
    from heterofl_amd.data import fetch_dataset, split_dataset
    from heterofl_amd.fed import FedRunner
    from heterofl_amd.fed.infer import NativeInference
    from heterofl_amd.logger import Logger
    from heterofl_amd.models import make_model
    from heterofl_amd.utils import process_dataset, make_optimizer
    cfg = make_cfg(base_cfg, '1_4_0.5_iid_fix_a1-e1_bn_1_1',
                   data_name='CIFAR10', model_name='resnet18')
    cfg['device'] = DEV
    cfg['engine'] = 'batched'
    torch.manual_seed(0)
    ds = fetch_dataset('CIFAR10', synthetic=True, synthetic_size=80)
    process_dataset(ds, cfg)
    data_split, label_split = split_dataset(ds, 4, 'iid', cfg['classes_size'])
    model = make_model(cfg).to(DEV)
    runner = FedRunner(cfg, ds, data_split, label_split, model,
                       make_optimizer(model, cfg['lr'], cfg),
                       logger=Logger(None))
    test_model = runner.stats()
    monkeypatch.delenv('HETEROFL_NATIVE_EVAL', raising=False)
    runner.test(test_model, 1)
    eager = dict(runner.logger.mean)
    runner.logger.reset()
    monkeypatch.setenv('HETEROFL_NATIVE_EVAL', '1')
    runner.test(test_model, 1)
    native = dict(runner.logger.mean)
    local, glob = runner._native_eval_sums(test_model)
    lsum = local.sum(0).tolist()
    glob = glob.tolist()
    want = {'test/Local-Loss': lsum[0] / lsum[2],
            'test/Local-Accuracy': 100.0 * lsum[1] / lsum[2],
            'test/Global-Loss': glob[0] / glob[2],
            'test/Global-Accuracy': 100.0 * glob[1] / glob[2]}
    img, _, aug = runner._stage_eval()
    x = aug(img, train=False)
    dlogit = (NativeInference(test_model)(x)
              - _eager_logits(test_model, x)).abs().max().item()
    for k, v in want.items():
        assert native[k] == pytest.approx(v, rel=1e-6, abs=1e-9), k
        if 'Loss' in k:
            print(k, 'native', native[k], 'eager', eager[k], 'max|dlogit|',
                  dlogit)
            assert abs(native[k] - eager[k]) <= 2.0 * dlogit + 1e-6, k
