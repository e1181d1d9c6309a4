"""Lite-Mono-8M depth encoder (reference networks/depth_encoder.py:9-431), restated without timm.

Three stages (dims 64/128/224, depths 4/4/10) of dilated depth-wise conv blocks, each closed by an LGFI
block (cross-covariance attention over channels + inverted bottleneck); an average-pooled copy of the
normalised input is concatenated before every down-sampling conv.  Parameter names are the reference's
 so `depth_enc.pth` checkpoints load unchanged.  All GEMM-shaped work (1x1 / 3x3
convs, Linear, attention matmuls) runs on MIOpen / hipBLASLt through PyTorch-ROCm.
"""
import math
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .layers import BatchNorm2d, Conv2d, conv_cat_aligned, stock_slices


class DropPath(nn.Module):
    """Stochastic depth per sample (the timm layer the reference imports at depth_encoder.py:7)."""

    def __init__(self, drop_prob=0.0):
        super().__init__()
        self.drop_prob = float(drop_prob)

    def forward(self, x):
        if self.drop_prob == 0.0 or not self.training:
            return x
        return x * self.sample_mask(x)

    def sample_mask(self, x):
        """The per-sample keep/scale factors (B,1,..,1) of one training forward; None when the layer is inactive."""
        if self.drop_prob == 0.0 or not self.training:
            return None
        pre = getattr(self, "_predrawn", None)
        if pre is not None:                       # drawn for all blocks of this forward at once (LiteMono.draw_drop_masks)
            self._predrawn = None
            if pre.shape[0] == x.shape[0] and pre.device == x.device:       # (drawn in fp32; under autocast x may be half)
                return pre.to(x.dtype).view((x.shape[0],) + (1,) * (x.ndim - 1))
        keep = 1.0 - self.drop_prob
        mask = x.new_empty((x.shape[0],) + (1,) * (x.ndim - 1)).bernoulli_(keep)
        if keep > 0.0:
            mask.div_(keep)
        return mask


class PositionalEncodingFourier(nn.Module):
    def __init__(self, hidden_dim=32, dim=768, temperature=10000):
        super().__init__()
        self.token_projection = nn.Conv2d(hidden_dim * 2, dim, kernel_size=1)
        self.scale = 2 * math.pi
        self.temperature, self.hidden_dim, self.dim = temperature, hidden_dim, dim

    def forward(self, B, H, W):
        return self.token_projection(self.features(B, H, W))

    def features(self, B, H, W):
        """The fixed sin/cos grid (B, 2*hidden, H, W) in front of the learned projection: a function of the shape only, so it is
        built once per (shape, device) instead of with ~25 small kernels in every forward."""
        dev = self.token_projection.weight.device
        # ... and per stream, like _eye below (round 5 audit of tensors that cross streams without an event, VERDICT r4 next #1c): the
        # depth passes of one step run on two streams; a copy made on one must not be read by the other while it is being filled
        stream = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0
        key = (B, H, W, str(dev), stream)
        if getattr(self, "_feat_cache", None) is None:
            self._feat_cache = {}
        if key not in self._feat_cache:
            with torch.no_grad():
                self._feat_cache[key] = self._build_features(B, H, W, dev)
        return self._feat_cache[key]

    def _build_features(self, B, H, W, dev):
        ones = torch.ones(B, H, W, dtype=torch.float32, device=dev)
        y_embed, x_embed = ones.cumsum(1), ones.cumsum(2)
        eps = 1e-6
        y_embed = y_embed / (y_embed[:, -1:, :] + eps) * self.scale
        x_embed = x_embed / (x_embed[:, :, -1:] + eps) * self.scale
        dim_t = torch.arange(self.hidden_dim, dtype=torch.float32, device=dev)
        dim_t = self.temperature ** (2 * torch.div(dim_t, 2, rounding_mode="trunc") / self.hidden_dim)
        pos_x = x_embed[:, :, :, None] / dim_t
        pos_y = y_embed[:, :, :, None] / dim_t
        pos_x = torch.stack((pos_x[..., 0::2].sin(), pos_x[..., 1::2].cos()), dim=4).flatten(3)
        pos_y = torch.stack((pos_y[..., 0::2].sin(), pos_y[..., 1::2].cos()), dim=4).flatten(3)
        return torch.cat((pos_y, pos_x), dim=3).permute(0, 3, 1, 2)


_EYES = {}


def _eye(n, dtype, device):
    """torch.eye(n), made once per (n, dtype, device, stream): a constant (two launches per attention block and step otherwise).
    Per stream: the depth passes of one step run on several streams, and a stream must not read what another is still filling."""
    stream = torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else 0
    key = (n, dtype, str(device), stream)
    e = _EYES.get(key)
    if e is None or stock_slices("eye"):
        e = _EYES[key] = torch.eye(n, dtype=dtype, device=device)
    return e


class XCA(nn.Module):
    """Cross-covariance attention: softmax over the (d_h x d_h) channel covariance of l2-normalised q, k."""

    def __init__(self, dim, num_heads=8, qkv_bias=False, qk_scale=None, attn_drop=0.0, proj_drop=0.0):
        super().__init__()
        self.num_heads = num_heads
        self.temperature = nn.Parameter(torch.ones(num_heads, 1, 1))
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)

    @staticmethod
    def _linear(layer, x, hw):
        """layer(x) for tokens (B,N,C); with the (H,W) of the token grid known, through the channels-last Linear whose weight
        and bias gradient come from one pass of dd_linear_wgrad (K = B*N = 92 160 rows against a 64 x 192 result: 300 us as a plain GEMM)."""
        if hw is not None and x.is_cuda and layer.bias is not None and os.environ.get("DD_STOCK_LINEAR_GRAD", "0") != "1":
            from hipops.functions import pointwise_linear
            B, N, Cc = x.shape
            return pointwise_linear(x.reshape(B, hw[0], hw[1], Cc), layer).reshape(B, N, layer.out_features)
        return layer(x)

    def forward(self, x, hw=None):
        """Cross-covariance attention (reference networks/depth_encoder.py:73-98): per head, softmax over channels of
        normalize(q) normalize(k)^T * temperature, applied to v.  Same arithmetic, GEMM-friendly order: the reference permutes
        q, k, v to (B,heads,d,N) -- three full-size layout copies -- and L2-normalises q and k along the N tokens (two strided
        reductions + two full-size divisions).  Here the Gram matrix q^T k is one batched GEMM straight on the (B,N,3C) `qkv`
        buffer (operands are strided views, all heads at once; only the d x d diagonal blocks are used), the normalisation
        divides the small Gram blocks by the outer product of the column norms, and attn @ v is one GEMM with the
        block-diagonal (C x C) attention matrix that writes (B,N,C) directly."""
        B, N, Cc = x.shape
        H, d = self.num_heads, Cc // self.num_heads
        if os.environ.get("DD_STOCK_XCA", "0") == "1":                       # the reference's operation order, for A/B runs
            qkv = self.qkv(x).reshape(B, N, 3, H, d).permute(2, 0, 3, 4, 1)  # (3,B,heads,d,N)
            q, k, v = F.normalize(qkv[0], dim=-1), F.normalize(qkv[1], dim=-1), qkv[2]
            attn = self.attn_drop(((q @ k.transpose(-2, -1)) * self.temperature).softmax(dim=-1))
            return self.proj_drop(self.proj((attn @ v).permute(0, 3, 1, 2).reshape(B, N, Cc)))
        qkv = self._linear(self.qkv, x, hw)                                  # (B,N,3C)
        if torch.is_grad_enabled() and qkv.requires_grad and not stock_slices("qkv"):
            from hipops.functions import SplitQKVFn              # the same views; their backward is one concatenation
            q, k, v, qk = SplitQKVFn.apply(qkv, Cc)
        else:
            q, k, v, qk = qkv[:, :, :Cc], qkv[:, :, Cc:2 * Cc], qkv[:, :, 2 * Cc:], qkv[:, :, :2 * Cc]   # strided views, no copies
        norms = torch.linalg.vector_norm(qk, dim=1).clamp_min(1e-12)          # (B,2C): F.normalize's eps
        gram = torch.bmm(q.transpose(1, 2), k).view(B, H, d, H, d)           # (B,C,C): all head pairs; keep h == h'
        gram = torch.diagonal(gram, dim1=1, dim2=3).permute(0, 3, 1, 2)      # (B,H,d,d) view
        scale = norms[:, :Cc].reshape(B, H, d, 1) * norms[:, Cc:].reshape(B, H, 1, d)
        attn = self.attn_drop(((gram / scale) * self.temperature).softmax(dim=-1))                # (B,H,d,d)
        eye = _eye(H, attn.dtype, attn.device).view(1, H, 1, H, 1)
        block = (attn.transpose(-1, -2).unsqueeze(3) * eye).reshape(B, Cc, Cc)                   # block-diagonal, [c', c]
        return self.proj_drop(self._linear(self.proj, torch.bmm(v, block), hw))   # out[n,(h,i)] = sum_j attn[h,i,j] v[n,(h,j)]


class LayerNorm(nn.Module):
    def __init__(self, normalized_shape, eps=1e-6, data_format="channels_last"):
        super().__init__()
        if data_format not in ("channels_last", "channels_first"):
            raise NotImplementedError
        self.weight = nn.Parameter(torch.ones(normalized_shape))
        self.bias = nn.Parameter(torch.zeros(normalized_shape))
        self.eps, self.data_format, self.normalized_shape = eps, data_format, (normalized_shape,)

    def forward(self, x):
        if self.data_format == "channels_last":
            if x.is_cuda and os.environ.get("DD_STOCK_LAYERNORM", "0") != "1":
                from hipops.functions import layer_norm_last      # rows of 64-224 floats: a lane group per row
                return layer_norm_last(x, self.weight, self.bias, self.eps)
            return F.layer_norm(x, self.normalized_shape, self.weight, self.bias, self.eps)
        u = x.mean(1, keepdim=True)
        s = (x - u).pow(2).mean(1, keepdim=True)
        x = (x - u) / torch.sqrt(s + self.eps)
        return self.weight[:, None, None] * x + self.bias[:, None, None]


class BNGELU(nn.Module):
    def __init__(self, nIn):
        super().__init__()
        self.bn = BatchNorm2d(nIn, eps=1e-5)
        self.act = nn.GELU()

    def forward(self, x):
        return self.bn(x, act="gelu")


class Conv(nn.Module):
    def __init__(self, nIn, nOut, kSize, stride, padding=0, dilation=(1, 1), groups=1, bn_act=False, bias=False):
        super().__init__()
        self.bn_act = bn_act
        # layers.Conv2d = nn.Conv2d (same keys); its 3x3 stride-1 instances on 16+ channels (the stem) run through dd_conv3x3_mfma
        self.conv = Conv2d(nIn, nOut, kernel_size=kSize, stride=stride, padding=padding, dilation=dilation, groups=groups, bias=bias)
        if bn_act:
            self.bn_gelu = BNGELU(nOut)

    def forward(self, x):
        x = self.conv(x)
        return self.bn_gelu(x) if self.bn_act else x

    def forward_cat(self, parts):
        """forward(torch.cat(parts, 1)) with the concatenation padded to an aligned channel count on the GPU."""
        x = conv_cat_aligned(self.conv, parts)
        return self.bn_gelu(x) if self.bn_act else x


class CDilated(nn.Module):
    def __init__(self, nIn, nOut, kSize, stride=1, d=1, groups=1, bias=False):
        super().__init__()
        self.conv = nn.Conv2d(nIn, nOut, kSize, stride=stride, padding=int((kSize - 1) / 2) * d, bias=bias, dilation=d, groups=groups)

    def forward(self, x):
        c = self.conv
        if (x.is_cuda and c.groups == c.in_channels == c.out_channels and c.kernel_size == (3, 3) and c.stride == (1, 1)
                and c.bias is None and c.padding == c.dilation and c.dilation[0] == c.dilation[1]
                and os.environ.get("DD_STOCK_DWCONV", "0") != "1"):
            from hipops.functions import depthwise_conv3x3       # MIOpen has no dilated grouped convolution
            return depthwise_conv3x3(x, c.weight, c.dilation[0])
        return c(x)


def _mlp_residual(block, y, res):
    """res + drop_path(gamma * pwconv2(GELU(pwconv1(y)))), everything channels-last: y, res (B,H,W,C).
    The two Linears see a 2-D matrix (one GEMM with the bias in its epilogue) and layer scale, stochastic depth and the
    residual are one addcmul instead of three element-wise passes."""
    B, H, W, Cc = y.shape
    if y.is_cuda and os.environ.get("DD_STOCK_LINEAR_GRAD", "0") != "1":
        from hipops.functions import (mlp, mlp_fused, mlp_fused_ok, mlp_ok, mlp_recompute, mlp_recompute_ok, mlp_train, mlp_train_narrow,
                                      mlp_train_narrow_ok, mlp_train_ok, pointwise_linear)
        y = y.contiguous()
        if mlp_fused_ok(y, block):
            y = mlp_fused(y, block)                            # forward-only pass: the whole block in one kernel, hidden tile on chip
        elif mlp_train_ok(y, block):
            y = mlp_train(y, block)                            # stage 3 with a tape: the same kernel saves GELU and GELU', fused data gradient
        elif mlp_recompute_ok(y, block):
            y = mlp_recompute(y, block)                        # training pass: the same kernel forward, the hidden tensor rebuilt in the backward
        elif mlp_ok(y, block):
            y = mlp(y, block)                                  # csrc/dd_pw_gemm.hip: both Linears on the bf16 matrix pipe (fp32 accuracy), GELU in the second one's prologue
        elif mlp_train_narrow_ok(y, block):
            y = mlp_train_narrow(y, block)                     # stages 1 and 2 with a tape: mlp_train's design at C = 64 / 128 (behind the two opt-ins)
        else:                                                  # weight + bias gradient: one pass of dd_linear_wgrad
            y = pointwise_linear(block.act(pointwise_linear(y, block.pwconv1)), block.pwconv2)
    else:
        y = block.pwconv2(block.act(block.pwconv1(y.reshape(-1, Cc)))).reshape(B, H, W, Cc)
    drop = block.drop_path.sample_mask(y) if isinstance(block.drop_path, DropPath) else None
    if block.gamma is None:
        return res + (y if drop is None else y * drop)
    if y.is_cuda and os.environ.get("DD_STOCK_LAYER_SCALE", "0") != "1":
        from hipops.functions import layer_scale_residual
        return layer_scale_residual(res, y, block.gamma, drop)
    return torch.addcmul(res, y, block.gamma if drop is None else block.gamma * drop)


class DilatedConv(nn.Module):
    """Depth-wise dilated 3x3 -> BN -> (channels-last) Linear 6x -> GELU -> Linear -> layer scale -> drop path.
    `norm` exists (and is in the checkpoints) but the reference never applies it (depth_encoder.py:205-220)."""

    def __init__(self, dim, k, dilation=1, stride=1, drop_path=0.0, layer_scale_init_value=1e-6, expan_ratio=6):
        super().__init__()
        self.ddwconv = CDilated(dim, dim, kSize=k, stride=stride, groups=dim, d=dilation)
        self.bn1 = BatchNorm2d(dim)
        self.norm = LayerNorm(dim, eps=1e-6)
        self.pwconv1 = nn.Linear(dim, expan_ratio * dim)
        self.act = nn.GELU()
        self.pwconv2 = nn.Linear(expan_ratio * dim, dim)
        self.gamma = nn.Parameter(layer_scale_init_value * torch.ones(dim), requires_grad=True) if layer_scale_init_value > 0 else None
        self.drop_path = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()

    def forward(self, x):
        y = self.bn1(self.ddwconv(x)).permute(0, 2, 3, 1)
        return _mlp_residual(self, y, x.permute(0, 2, 3, 1)).permute(0, 3, 1, 2)


class LGFI(nn.Module):
    """Local-global feature interaction: x += gamma_xca * XCA(LN(x + pos)); then LN -> MLP -> layer scale."""

    def __init__(self, dim, drop_path=0.0, layer_scale_init_value=1e-6, expan_ratio=6, use_pos_emb=True, num_heads=6,
                 qkv_bias=True, attn_drop=0.0, drop=0.0):
        super().__init__()
        self.dim = dim
        self.pos_embd = PositionalEncodingFourier(dim=dim) if use_pos_emb else None
        self.norm_xca = LayerNorm(dim, eps=1e-6)
        self.gamma_xca = nn.Parameter(layer_scale_init_value * torch.ones(dim), requires_grad=True) if layer_scale_init_value > 0 else None
        self.xca = XCA(dim, num_heads=num_heads, qkv_bias=qkv_bias, attn_drop=attn_drop, proj_drop=drop)
        self.norm = LayerNorm(dim, eps=1e-6)
        self.pwconv1 = nn.Linear(dim, expan_ratio * dim)
        self.act = nn.GELU()
        self.pwconv2 = nn.Linear(expan_ratio * dim, dim)
        self.gamma = nn.Parameter(layer_scale_init_value * torch.ones(dim), requires_grad=True) if layer_scale_init_value > 0 else None
        self.drop_path = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()

    def forward(self, x):
        B, Cc, H, W = x.shape
        t = x.reshape(B, Cc, H * W).permute(0, 2, 1)
        if self.pos_embd:
            t = t + self.pos_embd(B, H, W).reshape(B, -1, t.shape[1]).permute(0, 2, 1)
        a = self.xca(self.norm_xca(t), hw=(H, W))
        t = t + a if self.gamma_xca is None else torch.addcmul(t, a, self.gamma_xca)
        return _mlp_residual(self, self.norm(t.reshape(B, H, W, Cc)), x.permute(0, 2, 3, 1)).permute(0, 3, 1, 2)


class AvgPool(nn.Module):
    def __init__(self, ratio):
        super().__init__()
        self.pool = nn.ModuleList([nn.AvgPool2d(3, stride=2, padding=1) for _ in range(ratio)])

    def forward(self, x):
        for p in self.pool:
            x = p(x)
        return x


class LiteMono(nn.Module):
    def __init__(self, in_chans=3, model="lite-mono-8m", global_block=[1, 1, 1], global_block_type=["LGFI", "LGFI", "LGFI"],
                 drop_path_rate=0.2, layer_scale_init_value=1e-6, expan_ratio=6, heads=[8, 8, 8],
                 use_pos_embd_xca=[True, False, False], pretrained=True, **kwargs):
        super().__init__()
        assert model == "lite-mono-8m", "Only using lite-mono-8m"
        self.num_ch_enc = np.array([64, 128, 224])
        self.depth = [4, 4, 10]
        self.dims = [64, 128, 224]
        self.dilation = [[1, 2, 3], [1, 2, 3], [1, 2, 3, 1, 2, 3, 2, 4, 6]]
        for g in global_block_type:
            assert g in ("None", "LGFI")
        d0 = self.dims[0]
        self.downsample_layers = nn.ModuleList([nn.Sequential(
            Conv(in_chans, d0, kSize=3, stride=2, padding=1, bn_act=True),
            Conv(d0, d0, kSize=3, stride=1, padding=1, bn_act=True),
            Conv(d0, d0, kSize=3, stride=1, padding=1, bn_act=True))])
        self.stem2 = nn.Sequential(Conv(d0 + 3, d0, kSize=3, stride=2, padding=1, bn_act=False))
        self.input_downsample = nn.ModuleList([AvgPool(i) for i in range(1, 5)])
        for i in range(2):
            self.downsample_layers.append(nn.Sequential(
                Conv(self.dims[i] * 2 + 3, self.dims[i + 1], kSize=3, stride=2, padding=1, bn_act=False)))
        rates = [r.item() for r in torch.linspace(0, drop_path_rate, sum(self.depth))]
        self.stages = nn.ModuleList()
        first = 0
        for i, nblocks in enumerate(self.depth):
            blocks = []
            for j in range(nblocks):
                if j > nblocks - global_block[i] - 1:
                    if global_block_type[i] != "LGFI":
                        raise NotImplementedError
                    blocks.append(LGFI(dim=self.dims[i], drop_path=rates[first + j], expan_ratio=expan_ratio,
                                       use_pos_emb=use_pos_embd_xca[i], num_heads=heads[i],
                                       layer_scale_init_value=layer_scale_init_value))
                else:
                    blocks.append(DilatedConv(dim=self.dims[i], k=3, dilation=self.dilation[i][j], drop_path=rates[first + j],
                                              layer_scale_init_value=layer_scale_init_value, expan_ratio=expan_ratio))
            self.stages.append(nn.Sequential(*blocks))
            first += nblocks
        self.apply(self._init_weights)
        if pretrained:
            self.load_pretrained_model(model)

    @staticmethod
    def _init_weights(m):
        if isinstance(m, (nn.Conv2d, nn.Linear)):
            nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
        elif isinstance(m, (LayerNorm, nn.LayerNorm)):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)
        elif isinstance(m, nn.BatchNorm2d):
            nn.init.constant_(m.weight, 1)
            nn.init.constant_(m.bias, 0)

    def load_pretrained_model(self, model_name, dev="cpu"):
        path = "./ckpt/{}-pretrain.pth".format(model_name)
        if not os.path.exists(path):
            raise FileNotFoundError("{} not found and there is no network to fetch it; use --weights_init scratch".format(path))
        own = self.state_dict()
        loaded = torch.load(path, map_location=dev)["model"]
        own.update({k: v for k, v in loaded.items() if k in own and not k.startswith("norm")})
        self.load_state_dict(own)

    def draw_drop_masks(self, x, install=True):
        """Stochastic depth for every block of one forward in three kernels instead of two per block (51 blocks per training
        step): one uniform draw of (blocks, B), compared with each block's keep probability and divided by it.  Same
        distribution as per-block `bernoulli_(keep) / keep`; the position in the random stream differs.
        install=False only returns the (blocks, B) factors: networks.Model draws the masks of its three depth passes up front,
        in frame order, so that issuing the passes on separate streams does not permute the random stream among the frames."""
        if not self.training:
            return
        layers = getattr(self, "_drop_layers", None)
        if layers is None:
            layers = self._drop_layers = [m for m in self.modules() if isinstance(m, DropPath) and m.drop_prob > 0.0]
        if not layers:
            return
        keep = getattr(self, "_keep_probs", None)
        if keep is None or keep.device != x.device or keep.shape[0] != len(layers):
            keep = torch.tensor([1.0 - m.drop_prob for m in layers], dtype=torch.float32, device=x.device).view(-1, 1)
            self._keep_probs = keep
        masks = (torch.rand(len(layers), x.shape[0], dtype=torch.float32, device=x.device) < keep).to(x.dtype) / keep
        if install:
            for m, row in zip(layers, masks.unbind(0)):
                m._predrawn = row
        return masks

    def install_drop_masks(self, masks):
        """The next forward uses these factors instead of drawing its own."""
        for m, row in zip(self._drop_layers, masks.unbind(0)):
            m._predrawn = row
        self._masks_installed = True

    def forward_features(self, x):
        if x.is_cuda and os.environ.get("DD_STOCK_DROP_PATH", "0") != "1":
            if getattr(self, "_masks_installed", False):
                self._masks_installed = False
            else:
                self.draw_drop_masks(x)
        x = (x - 0.45) / 0.225
        stem = self.downsample_layers[0][0].conv.weight
        if stem.is_contiguous(memory_format=torch.channels_last) and not stem.is_contiguous():
            # channels-last model: keep the pooled copies of the input (and the cats they enter) channels-last as well
            x = x.contiguous(memory_format=torch.channels_last)
        # input_downsample[i] is i+1 identical 3x3/stride-2 average pools applied to x (reference depth_encoder.py:278-289,329-331,400);
        # chaining them is the same arithmetic with 3 kernels instead of 10 (the 4-fold pool is never consumed)
        pooled = [self.input_downsample[0](x)]
        for _ in (1, 2):
            pooled.append(self.input_downsample[0](pooled[-1]))
        feats = []
        x = self.stem2[0].forward_cat((self.downsample_layers[0](x), pooled[0]))
        carry = [x]
        x = self.stages[0](x)
        carry.append(x)
        feats.append(x)
        for i in (1, 2):
            carry.append(pooled[i])
            x = self.downsample_layers[i][0].forward_cat(carry)
            carry = [x]
            x = self.stages[i](x)
            carry.append(x)
            feats.append(x)
        return feats

    def forward(self, x):
        return self.forward_features(x)
