"""`build_model` and `ModelWrapper` (torchdet3d/builders/model_builder.py:25-151) over the HIP engine.

Same call surface as the reference: `build_model(config, export_mode=False, weights_path='')` returns an
`nn.Module` whose `forward(x, cats) -> (kp [B,9,2], targets [B,num_classes] | cats[:,None])`, with
`train()/eval()/to()/parameters()/state_dict()/load_state_dict()` (state-dict keys and shapes are the
reference's).  Differences a caller can observe:
  * `parameters()` yields ONE flat fp32 tensor holding every weight (the named tensors are views into it), so an
    optimizer built by `build_optimizer` is a single fused update and data-parallel training all-reduces one
    buffer; `named_parameters()` therefore has one entry, `state_dict()` keeps the per-layer names;
  * the forward runs on the GPU only ('--device cuda'); there is no CPU fallback;
  * model names: of the reference's six, 'mobilenetv3_large', 'mobilenetv3_small' and 'mobilenetv3_large_21k' (its default
    config's model: timm's mobilenetv3_large_100 restated in models/arch.py -- timm is installed nowhere this project is
    built or tested, so the layout, key names and initialisation are UNPINNED against timm itself; the parameter count and
    everything shared with the reference's own class are pinned).  'efficientnet-lite0/1/2' are not built: no source of the
    efficientnet_lite_pytorch package exists to restate, and they need TF-"same" asymmetric padding, BatchNorm eps 1e-3 and
    stochastic depth in training (an RNG contract of its own).  Extra names: 'mobilenetv2' (north-star throughput model) and
    'resnet50' (BASELINE config 4; standard torchvision architecture, models/resnet.py).
  * `regressors`, `cls_fc`, `sigmoid` (model_builder.py:79-87) are views onto the flat buffer, `extract_features`
    (mobilenetv3.py:199-203) and `_glob_feature_vector` (:96-110) are callable but inference-only: training goes
    through `forward`, whose whole graph is one autograd node;
  * a train-mode model called under `torch.no_grad()` behaves like the reference's: batch statistics, running
    estimates updated, dropout applied -- only the activations are not kept for a backward.
Config keys read: model.name, model.num_classes, model.pretrained (never touches the network: 'mobilenetv3_large_21k' loads
$TORCH_HOME/checkpoints/mobilenetv3_large_21k_imagenet.pth -- the file the reference's init_pretrained_weights caches -- when
it exists and says so in one line when it does not; ignored for the other names), model.load_weights,
model.storage_dtype ('f32' default for parity | 'bf16' throughput mode), model.eval_storage_dtype (storage precision of
eval-mode forwards; default 'f32' also for a 'bf16' model, so that inference outputs meet the 1e-4 parity bound; 'f16': fp16
activation storage, the fast option that is INSIDE the 1e-3 3-D-IoU / ADD bounds for mobilenetv2 (keypoints 1.7e-4, 2.3x the
fp32 engine's throughput); 'bf16': inference in the training precision, outside the IoU bound for mobilenetv2), model.pooling_mode ('avg' | 'max' |
'avg+max'; the reference fixes this at its default 'avg', model_builder.py:73-74)."""
import os

import torch
import torch.distributed as dist
from torch import nn

from ..models.arch import AVAILABLE_MODELS
from ..models.engine import Net
from ..models.resnet import ResNetEngine
from ..utils.utils import load_pretrained_weights


class _Run(torch.autograd.Function):
    """The whole network as one autograd node: forward = engine.forward, backward = engine.backward."""

    @staticmethod
    def forward(ctx, flat, wrapper, x, cats, mask, train):
        net = wrapper.net
        kp, logits = net.forward(x, cats, train=train, dropout_mask=mask)
        ctx.wrapper, ctx.train, ctx.generation = wrapper, train, net.generation
        if logits is None:
            logits = torch.empty(0, device=kp.device)
            ctx.mark_non_differentiable(logits)
        return kp, logits

    @staticmethod
    def backward(ctx, dkp, dlogits):
        net = ctx.wrapper.net
        if not ctx.train:
            raise RuntimeError('backward through an eval-mode forward is not supported (BatchNorm uses running stats)')
        if net.saved is None or net.saved.get('generation') != ctx.generation:
            # the engine keeps the activations of ONE train-mode forward (the latest); back-propagating an older
            # forward through them would silently produce the wrong gradients
            raise RuntimeError('backward() of a forward whose activations were overwritten by a later train-mode '
                               'forward (or already consumed): run forward -> backward one batch at a time')
        if dkp is None:
            dkp = torch.zeros(net.saved['B'], 9, 2, device=net.device)
        if net.num_classes > 1 and dlogits is None:
            dlogits = torch.zeros(net.saved['B'], net.num_classes, device=net.device)
        sync = ctx.wrapper.grad_sync
        if sync is not None:
            sync.start()
        net.backward(dkp.contiguous(), dlogits.contiguous() if net.num_classes > 1 else None)
        if sync is not None:
            sync.finish()
        return net.gflat, None, None, None, None, None


class _HeadView(nn.Module):
    """`regressors[k][0]` / `cls_fc[1]` as a caller of the reference sees them (model_builder.py:79-85): a Linear whose
    weight / bias are VIEWS into the engine's flat master buffer (not separately registered parameters: the optimizer
    keeps seeing the one flat tensor).  Calling it runs the product's GEMM kernel."""

    def __init__(self, wrapper, wkey, bkey):
        super().__init__()
        object.__setattr__(self, '_w', wrapper)
        self._wkey, self._bkey = wkey, bkey

    @property
    def weight(self):
        return self._w.net.p[self._wkey]

    @property
    def bias(self):
        return self._w.net.p[self._bkey]

    @property
    def in_features(self):
        return self.weight.shape[1]

    @property
    def out_features(self):
        return self.weight.shape[0]

    @torch.no_grad()
    def forward(self, x):
        from .. import _native as N
        squeeze = x.dim() == 1
        x2 = x.reshape(-1, x.shape[-1]).float().contiguous()
        if not x2.is_cuda:
            raise RuntimeError('the HIP path needs its inputs on the GPU (no CPU fallback)')
        w, b = self.weight, self.bias
        y = torch.empty(x2.shape[0], w.shape[0], device=x2.device)
        N.call('t3d_linear_fwd', N.ptr(x2), N.ptr(w.contiguous()), N.ptr(b.contiguous()), N.ptr(y), x2.shape[0],
               w.shape[1], w.shape[0], N.stream())
        return y[0] if squeeze else y.view(*x.shape[:-1], w.shape[0])


class _Sigmoid(nn.Module):
    """`self.sigmoid` (model_builder.py:87); inside `forward` the sigmoid is fused into the head kernel."""

    def forward(self, x):
        return torch.sigmoid(x)


class ModelWrapper(nn.Module):
    def __init__(self, name, num_classes=9, export_mode=False, storage_dtype='f32', device='cpu', pooling_mode='avg',
                 eval_storage_dtype=None):
        super().__init__()
        assert name in AVAILABLE_MODELS, f'Wrong model name parameter. Expected one of {AVAILABLE_MODELS}'
        if pooling_mode not in ('avg', 'max', 'avg+max'):
            raise ValueError(f'Unknown pooling mode: {pooling_mode}')          # model_builder.py:105-106
        self.name, self.num_classes, self.export_mode, self.pooling_mode = name, num_classes, export_mode, pooling_mode
        self.storage_dtype = torch.bfloat16 if storage_dtype in ('bf16', torch.bfloat16) else torch.float32
        # Inference precision.  The throughput mode ('bf16' storage) trains with bf16 activations; what the model RETURNS in
        # eval mode -- the outputs the parity bounds are about (keypoints 1e-4, class arg-max exact, 3-D IoU 1e-3) -- comes
        # from an fp32-storage engine over the same parameters unless the config asks for 'bf16' inference explicitly
        # (MobileNetV2's bf16 inference keypoints are 3e-4 rms off, which moves the ill-conditioned 3-D IoU by 2e-3 .. 4e-3:
        # tests/test_gpu_bf16_gate.py)
        if not eval_storage_dtype:
            eval_storage_dtype = 'f32' if self.storage_dtype == torch.bfloat16 else None
        # 'f16' (round 4): fp16 activation storage for inference -- bf16's bytes and speed with three more mantissa bits at every
        # MFMA operand; served for mobilenetv2 and mobilenetv3_large_21k (whose 5x5 depthwise and gated 1x1 forwards exist in fp16),
        # anything else falls back to 'f32'
        if eval_storage_dtype in ('f16', torch.float16) and name not in ('mobilenetv2', 'mobilenetv3_large_21k'):
            eval_storage_dtype = 'f32'
        self.eval_storage_dtype = (None if not eval_storage_dtype else
                                   torch.bfloat16 if eval_storage_dtype in ('bf16', torch.bfloat16) else
                                   torch.float16 if eval_storage_dtype in ('f16', torch.float16) else torch.float32)
        self.grad_sync = None          # optional torchdet3d.parallel.GradSync (one process per GPU)
        self.input_normalization = ([0.5931, 0.4690, 0.4229], [0.2471, 0.2214, 0.2157])   # configs/default_config.py:9-10
        self._make(torch.device(device))
        # the reference's head attributes (model_builder.py:79-87) as views; kept out of `_modules` / `_parameters`
        # so that parameters() stays the single flat tensor
        regs = [nn.Sequential(_HeadView(self, f'regressors.{k}.0.weight', f'regressors.{k}.0.bias')) for k in range(9)]
        object.__setattr__(self, '_regressors', nn.ModuleList(regs))
        object.__setattr__(self, '_cls_fc', nn.Sequential(nn.Dropout(0.5), _HeadView(self, 'cls_fc.1.weight', 'cls_fc.1.bias')))
        object.__setattr__(self, '_sigmoid', _Sigmoid())

    regressors = property(lambda self: self._regressors)
    cls_fc = property(lambda self: self._cls_fc)
    sigmoid = property(lambda self: self._sigmoid)

    def _make(self, device, state=None):
        engine = ResNetEngine if self.name == 'resnet50' else Net
        self.net = engine(self.name, self.num_classes, device, self.storage_dtype, self.pooling_mode)
        if state is not None:
            self.net.load_state_dict(state)
        # optional second engine over the SAME parameters / BatchNorm buffers for eval-mode forwards in another storage
        # precision (fp32 validation of a bf16-trained model: the 3-D IoU then equals the fp32 path's)
        self.net_eval = self.net
        if self.eval_storage_dtype is not None and self.eval_storage_dtype != self.storage_dtype and device.type == 'cuda':
            self.net_eval = engine(self.name, self.num_classes, device, self.eval_storage_dtype, self.pooling_mode, share=self.net)
        self.set_input_normalization(*self.input_normalization)
        self.flat = nn.Parameter(self.net.flat)     # shares storage with the engine's master weights
        # one process per GPU (launched by torch.distributed.run): the gradient exchange attaches itself as soon as the
        # model sits on its GPU -- scripts/main.py needs no change (its nn.DataParallel branch, main.py:60-61, is what
        # this replaces; `cfg.data_parallel.use_parallel` stays False)
        if self.grad_sync is None and device.type == 'cuda' and dist.is_available() and dist.is_initialized() and \
                (dist.get_world_size() > 1 or os.environ.get('T3D_FORCE_SYNC')):
            self.grad_sync = True
        if self.grad_sync is not None and device.type == 'cuda':
            self.attach_grad_sync(self.grad_sync)

    def set_input_normalization(self, mean, std):
        """Mean / std applied to uint8 NHWC crops inside the stem's patch gather (configs/default_config.py:9-10; fp32 crops
        arrive normalised, as in the reference, and are not touched)."""
        self.input_normalization = (list(mean), list(std))
        for net in {id(self.net): self.net, id(self.net_eval): self.net_eval}.values():
            net.set_input_normalization(mean, std)

    @torch.no_grad()
    def extract_features(self, x):
        """mobilenetv3.py:199-203: activated last feature map, fp32 NCHW [B, C, H/32, W/32] (inference)."""
        if not x.is_cuda:
            raise RuntimeError('the HIP path needs the model and the crops on the GPU (no CPU fallback)')
        return self.net.extract_features(x.float())

    @staticmethod
    @torch.no_grad()
    def _glob_feature_vector(x, mode, reduce_dims=True):
        """model_builder.py:96-110 on an NCHW feature map: 'avg' | 'max' | 'avg+max', ValueError otherwise."""
        from .. import _native as N
        if mode not in N.POOL:
            raise ValueError(f'Unknown pooling mode: {mode}')
        if not x.is_cuda:
            raise RuntimeError('the HIP path needs its inputs on the GPU (no CPU fallback)')
        B, C, H, W = x.shape
        if C % 8:
            raise RuntimeError('channel count must be a multiple of 8')
        nhwc = x.float().permute(0, 2, 3, 1).contiguous()
        out = torch.empty(B, C, device=x.device)
        N.call('t3d_pool_fwd', N.F32, N.ptr(nhwc), None, N.POOL[mode], N.ptr(out), None, B, H * W, C, N.stream())
        return out if reduce_dims else out.view(B, C, 1, 1)

    def attach_grad_sync(self, sync_cls_or_obj):
        from ..parallel import GradSync
        self.grad_sync = GradSync(self.net.gflat) if sync_cls_or_obj is True else sync_cls_or_obj
        self.grad_sync.g = self.net.gflat
        self.net.grad_hook = self.grad_sync.ready
        self.net.seed_rank = dist.get_rank() if dist.is_initialized() else 0      # independent dropout masks per rank
        self.grad_sync.broadcast([self.net.flat] + list(self.net.buffers.values()))

    def _replicate_for_data_parallel(self):
        # nn.DataParallel(net, ...) (scripts/main.py:60-61) copies per-layer parameters to several devices from ONE process;
        # this model is a single flat parameter over one engine per process
        raise RuntimeError('this model runs one process per GPU (python -m torch.distributed.run --nproc-per-node N '
                           'scripts/main.py ...): set data_parallel.use_parallel = False; the RCCL gradient exchange '
                           'attaches itself when WORLD_SIZE > 1')

    # ---- nn.Module surface -------------------------------------------------------------------------
    def _apply(self, fn, recurse=True):
        probe = fn(torch.empty(0, device=self.net.device))
        if probe.device != self.net.device:
            self._make(probe.device, self.net.state_dict())
        return self

    def state_dict(self, *args, destination=None, prefix='', keep_vars=False):
        sd = self.net.state_dict()
        out = destination if destination is not None else {}
        for k, v in sd.items():
            out[prefix + k] = v
        return out

    def load_state_dict(self, state_dict, strict=True):
        self.net.load_state_dict(state_dict, strict=strict)
        return self

    def forward(self, x, cats=None, dropout_mask=None):
        if self.export_mode:
            return self.forward_to_onnx(x)
        if not x.is_cuda:
            raise RuntimeError('the HIP path needs the model and the crops on the GPU (no CPU fallback)')
        train = self.training
        # uint8 NHWC crops go to the stem kernel as they are (normalised there, bf16 storage); anything else as fp32 NCHW
        x = x if x.dtype == torch.uint8 else x.float()
        if train and not torch.is_grad_enabled():
            # `model.train()` under torch.no_grad(): the reference's modules still normalise with the BATCH statistics, update
            # the running estimates and apply dropout -- only autograd is off.  Same here: a train-mode forward whose saved
            # activations are dropped (no backward can follow).
            kp, logits = self.net.forward(x, cats, train=True, dropout_mask=dropout_mask)
            self.net.saved = None
            return kp, (logits if self.num_classes > 1 else cats.unsqueeze(1))
        if not train and (self.net_eval is not self.net or not torch.is_grad_enabled()):
            # eval-mode forward (validation / serving): no autograd node; replayed from a recorded plan by one host call where
            # the inputs allow it (trainer/step_plan.py: ForwardPlan)
            with torch.no_grad():
                fp = self._forward_plan()
                if fp is not None and fp.accepts(x, cats):
                    kp, logits = fp(x, cats)
                else:
                    kp, logits = self.net_eval.forward(x, cats, train=False)
            return kp, (logits if self.num_classes > 1 else cats.unsqueeze(1))
        kp, logits = _Run.apply(self.flat, self, x, cats, dropout_mask, train)
        targets = logits if self.num_classes > 1 else cats.unsqueeze(1)     # model_builder.py:141-144
        return kp, targets

    def _forward_plan(self):
        fp = self.__dict__.get('_fplan')
        if fp is None or fp.net is not self.net_eval:
            from ..trainer.step_plan import ForwardPlan
            fp = ForwardPlan(self.net_eval)
            object.__setattr__(self, '_fplan', fp)
        return fp

    @torch.no_grad()
    def forward_to_onnx(self, x):
        """All 9 heads (model_builder.py:112-124): kp [9,B,9,2] (sigmoid), class logits (or zeros(B)) -- ONE pass over
        the backbone, then every regressor on every sample in one launch (`t3d_head_fwd_all`)."""
        if not x.is_cuda:
            raise RuntimeError('the HIP path needs the model and the crops on the GPU (no CPU fallback)')
        # uint8 NHWC crops (the two-stage path, utils/ie_wrappers.py) are normalised inside the stem's patch gather
        kp, logits = self.net_eval.forward(x if x.dtype == torch.uint8 else x.float(), None, train=False, all_heads=True)
        return kp, (logits if self.num_classes > 1 else torch.zeros(x.shape[0], device=x.device))


def _init_distributed():
    """Launched by torch.distributed.run with more than one rank (WORLD_SIZE > 1) and no process group yet: bind this
    process to its GPU and join the RCCL group BEFORE anything else touches the device, so that an unchanged
    scripts/main.py (`net.to('cuda')`) trains data-parallel.  Replaces main.py:60-61."""
    if not dist.is_available() or dist.is_initialized():
        return
    world = int(os.environ.get('WORLD_SIZE', '1'))
    if world <= 1 and not os.environ.get('T3D_FORCE_SYNC'):
        return
    if 'RANK' not in os.environ or 'MASTER_ADDR' not in os.environ:
        return
    local = int(os.environ.get('LOCAL_RANK', '0'))
    if torch.cuda.device_count() > local:          # (device_count does not initialise the GPU)
        torch.cuda.set_device(local)
        dist.init_process_group('nccl', device_id=torch.device('cuda', local))
    else:
        dist.init_process_group('gloo')


PRETRAINED_CACHED = ('mobilenetv3_large_21k',)      # names whose `pretrained=True` looks for the reference's cached file


def _torch_home():
    """mobilenetv3.py:243-255."""
    return os.path.expanduser(os.getenv('TORCH_HOME', os.path.join(os.getenv('XDG_CACHE_HOME', '~/.cache'), 'torch')))


def _load_cached_pretrained(model, name):
    """`init_pretrained_weights(model, key=name, extra_prefix='model.')` (model_builder.py:68-69, mobilenetv3.py:234-271)
    WITHOUT its download: the cached checkpoint is loaded when it is there (bare timm keys -> `model.*`; name or shape
    mismatches such as the checkpoint's `classifier.*` are dropped), otherwise the model keeps its initialisation."""
    cached = os.path.join(_torch_home(), 'checkpoints', name + '_imagenet.pth')
    if os.path.isfile(cached):
        load_pretrained_weights(model, cached, extra_prefix='model.')
        return True
    print(f'** model.pretrained: "{cached}" not found and nothing is downloaded; training starts from the initialisation')
    return False


def build_model(config, export_mode=False, weights_path=''):
    _init_distributed()
    if config.data_parallel and config.data_parallel.use_parallel and \
            (int(os.environ.get('WORLD_SIZE', '1')) > 1 or (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1)):
        raise RuntimeError('data_parallel.use_parallel = True (nn.DataParallel, scripts/main.py:60-61) under a multi-process '
                           'launch: set it to False -- every rank already owns one GPU and the gradients are exchanged over RCCL')
    name = config.model.name
    assert name in AVAILABLE_MODELS, f'Wrong model name parameter. Expected one of {AVAILABLE_MODELS}'
    model = ModelWrapper(name, config.model.num_classes or 9, export_mode, config.model.storage_dtype or 'f32',
                         pooling_mode=config.model.pooling_mode or 'avg',
                         eval_storage_dtype=config.model.eval_storage_dtype or None)
    weights = config.model.load_weights or weights_path
    if weights:
        load_pretrained_weights(model, weights)
    elif config.model.pretrained and not export_mode and name in PRETRAINED_CACHED:
        _load_cached_pretrained(model, name)
    norm = getattr(getattr(config, 'data', None), 'normalization', None)
    if norm:
        model.set_input_normalization(norm.mean, norm.std)
    return model
