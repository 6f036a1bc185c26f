"""Float64 reference of the HiFi-GAN generator, written from its definition, and the table of generator shapes the sweep of
test_generator_shapes.py walks.

The generator (Kong et al. 2020, section 2.1 and figure 1): conv_pre (k = 7), then per upsampling stage leaky_relu(0.1) ->
ConvTranspose1d(stride u, kernel k, padding (k - u) // 2) -> the MEAN of the stage's ResBlocks, then leaky_relu(0.01) -> conv_post
(k = 7) -> tanh.  ResBlock1 per dilation d: x += conv_k,1(lrelu(conv_k,d(lrelu(x)))); ResBlock2 per dilation: x += conv_k,d(lrelu(x));
all convolutions 'same'-padded.  Evaluated with torch.nn.functional.conv1d / conv_transpose1d in float64 on the weight-norm-folded state
dict: it shares no code with oracle/zvx_oracle.py (NumPy im2col in f32) nor with the device, so it pins the oracle at every shape of the
table -- the golden fixtures pin it only at the named configurations.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F


def _t(a):
    return torch.as_tensor(np.asarray(a, np.float64))


def _same(k, d):
    return (k - 1) * d // 2


def generator_ref(mel, sd, h):
    """mel [n_mels, P], sd: folded state dict (weights.folded(weights.hifigan_state_dict(h))), h: the generator's config.json.
    Returns (wav float64 [P * prod(rates)], stages: the float64 [C_i, T_i] tensor behind each stage's ResBlock mean)."""
    w = {k: _t(v) for k, v in sd.items()}
    x = F.conv1d(_t(mel)[None], w["conv_pre.weight"], w["conv_pre.bias"], padding=3)
    rk, rd = h["resblock_kernel_sizes"], h["resblock_dilation_sizes"]
    nk = len(rk)
    stages = []
    for i, (u, k) in enumerate(zip(h["upsample_rates"], h["upsample_kernel_sizes"])):
        x = F.leaky_relu(x, 0.1)
        x = F.conv_transpose1d(x, w[f"ups.{i}.weight"], w[f"ups.{i}.bias"], stride=u, padding=(k - u) // 2)
        total = torch.zeros_like(x)
        for j in range(nk):
            p, y = f"resblocks.{i * nk + j}", x
            for t, d in enumerate(rd[j]):
                if h["resblock"] == "1":
                    z = F.conv1d(F.leaky_relu(y, 0.1), w[f"{p}.convs1.{t}.weight"], w[f"{p}.convs1.{t}.bias"], dilation=d, padding=_same(rk[j], d))
                    z = F.conv1d(F.leaky_relu(z, 0.1), w[f"{p}.convs2.{t}.weight"], w[f"{p}.convs2.{t}.bias"], padding=_same(rk[j], 1))
                else:
                    z = F.conv1d(F.leaky_relu(y, 0.1), w[f"{p}.convs.{t}.weight"], w[f"{p}.convs.{t}.bias"], dilation=d, padding=_same(rk[j], d))
                y = y + z
            total = total + y
        x = total / nk
        stages.append(x[0].numpy())
    x = F.leaky_relu(x, 0.01)
    x = torch.tanh(F.conv1d(x, w["conv_post.weight"], w["conv_post.bias"], padding=3))
    return x[0, 0].numpy(), stages


def manifest_tensor(manifest, blob, name):
    """The tensor `name` of a packed model (pack.pack_model's manifest text + f32 blob), or None."""
    for line in manifest.splitlines():
        f = line.split()
        if len(f) > 4 and f[0] == "tensor" and f[1] == name:
            dims = [int(d) for d in f[4:4 + int(f[3])]]
            off = int(f[4 + int(f[3])])
            return blob[off:off + int(np.prod(dims))].reshape(dims)
    return None


def polyphase_upsample(x, manifest, blob, i, u):
    """Stage i's ConvTranspose1d as the device evaluates it, in float64 from the PACKED tensors: out[t u + ph][co] = bias + sum over
    the stored taps of poly[tap][ph * Cout + co][:] . x[t + dv] with rows outside [0, T) zero; dv = -1, 0, +1 for voc.up{i}_w and, where
    the packer emitted them, (-1, 0) for the phases of _wlo and (0, +1) for those of _whi.  x [T][Cin] -> [T u][Cout]; a dict keyed
    "w" (and "lohi") -> result."""
    x = np.asarray(x, np.float64)
    T, cin = x.shape
    xp = np.zeros((T + 2, cin))
    xp[1:T + 1] = x
    bias = manifest_tensor(manifest, blob, f"voc.up{i}_b").astype(np.float64)

    def run(poly, dvs):
        acc = np.zeros((T, poly.shape[1]))
        for tap, dv in enumerate(dvs):
            acc += xp[1 + dv:1 + dv + T] @ poly[tap].astype(np.float64).T
        return acc

    full = run(manifest_tensor(manifest, blob, f"voc.up{i}_w"), (-1, 0, 1)) + bias
    cout = full.shape[1] // u
    out = {"w": full.reshape(T * u, cout)}
    lo, hi = manifest_tensor(manifest, blob, f"voc.up{i}_wlo"), manifest_tensor(manifest, blob, f"voc.up{i}_whi")
    if lo is not None:
        both = np.concatenate([run(lo, (-1, 0)), run(hi, (0, 1))], axis=1) + bias
        out["lohi"] = both.reshape(T * u, cout)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# The sweep: one entry per branch of the routing in zvx.hip (voc_domains, voc_upsample, voc_narrow_stage, voc_resblock, stage_close).
#   h        the generator's config.json
#   hop      audio.hop_size of the model it is packed with (prod of the rates)
#   pmax     frames of the longest utterance of the ragged batch [pmax, 1, pmax // 2]: 40 where a stage has 128 channels, else 12
#   refused  None: runs.  Otherwise {precision: (config.json field, manifest key)} the refusal has to name -- at pack_model and at zvx_create
#   mixed    a ResBlock1 stage of 128 channels runs in bf16 inside the half generator (voc_domains): check_wav's limits for that arithmetic
#   absent   variant-name prefixes that must not appear in the 16-bit context
# LAUNCHES (below the table): per case {precision: {kernel variant: launches}} of ONE vocode_mel call on the ragged batch, every fusion
# on, as recorded on the MI355X (profiles/generator_shape_sweep.txt): a routing change has to edit it knowingly
# ------------------------------------------------------------------------------------------------------------------------------
def _rb(kind, c0, rates, ks, rk, rd):
    return {"resblock": kind, "upsample_rates": list(rates), "upsample_kernel_sizes": list(ks), "upsample_initial_channel": c0,
            "resblock_kernel_sizes": list(rk), "resblock_dilation_sizes": [list(d) for d in rd]}


_NARROW = {"bf16": ("upsample_initial_channel", "voc_c0")}
_KSIZE = {"bf16": ("upsample_kernel_sizes", "voc_ksizes"), "f32": ("upsample_kernel_sizes", "voc_ksizes")}

SWEEP = {
    # a 4-channel last stage (K = 4): f32 runs it (4 floats = one 16-byte group); the 16-bit kernels and conv_post read 8 elements -> refused
    "c4_tail": dict(h=_rb("1", 64, (8, 8, 2, 2), (16, 16, 4, 4), (3, 7), [(1, 3, 5)] * 2), hop=256, pmax=12, refused=_NARROW),
    # stage_close(nk = 1): no running sum; two pairs per block with the dilations (1, 3), which resstream's compile-time sets do not hold at
    # k = 3: per-pair launches; narrowstage declines (nd != 3); k = 3u at Cin 128; _wlo / _whi at Cin 256; k = u (padding 0) at Cin 32; the
    # 128-channel ResBlock1 stage is the FIRST one (bf16 inside the half generator; the pair kernel under pairstream 3)
    "one_block": dict(h=_rb("1", 256, (4, 4, 4, 4), (8, 12, 6, 4), (3,), [(1, 3)]), hop=256, pmax=40, refused=None, mixed=True,
                      absent=("narrowstage_",)),
    # 1 / nk = 0.25; accumulate modes 2, 3, 3, 1; k = 5 / 9 outside the fused kernels' tap counts; narrowstage declines (nk > 3)
    "four_blocks": dict(h=_rb("1", 128, (8, 8, 4), (16, 16, 8), (3, 5, 7, 9), [(1, 3, 5)] * 4), hop=256, pmax=12, refused=None,
                        absent=("narrowstage_",)),
    # nd = 1: one pair per block (k = 11 with dilation 1, k = 3 with dilation 5: neither is a resstream set)
    "one_dilation": dict(h=_rb("1", 128, (8, 8, 4), (16, 16, 8), (11, 3), [(1,), (5,)]), hop=256, pmax=12, refused=None,
                         absent=("narrowstage_",)),
    # resstream's shorter chains AS whole blocks at C = 64: k = 7 with (1, 3) is the two-pair chain (here it writes the running sum instead
    # of handing on to a third pair), k = 11 with (5) the one-pair chain (here it reads the stage input and closes the stage)
    "stream_tails": dict(h=_rb("1", 128, (8, 8, 4), (16, 16, 8), (7, 11), [(1, 3), (5,)]), hop=256, pmax=12, refused=None,
                         absent=("narrowstage_",)),
    # ResBlock2 with nd = 3: rb2fuse (two convolutions) must decline; u = 16 polyphase, N = 1024; four blocks
    "rb2_three": dict(h=_rb("2", 128, (16, 16), (32, 32), (3, 5, 7, 9), [(1, 2, 3)] * 4), hop=256, pmax=12, refused=None,
                      absent=("rb2fuse_",)),
    # ResBlock2 with nd = 1, nk = 1: every stage is ONE convolution that closes it
    "rb2_one": dict(h=_rb("2", 64, (8, 8, 4), (16, 16, 8), (3,), [(4,)]), hop=256, pmax=12, refused=None, absent=("rb2fuse_",)),
    # odd u, odd k with k - u even; hop 240; no _wlo / _whi; narrowstage at C = 16 / 8 behind odd row counts
    "odd_rates": dict(h=_rb("1", 128, (5, 3, 4, 4), (11, 7, 8, 8), (3, 7), [(1, 3, 5)] * 2), hop=240, pmax=12, refused=None),
    # k - u odd: torch's ConvTranspose1d yields T u + 1 rows
    "odd_k_minus_u": dict(h=_rb("1", 64, (8, 8, 4), (15, 16, 8), (3, 7), [(1, 3, 5)] * 2), hop=256, pmax=12, refused=_KSIZE),
    # k > 3u: the three polyphase taps do not cover the kernel
    "wide_k": dict(h=_rb("1", 64, (8, 8, 4), (32, 16, 8), (3, 7), [(1, 3, 5)] * 2), hop=256, pmax=12, refused=_KSIZE),
}

LAUNCHES = {'c4_tail': {'f32': {'gemm_f32_256x32': 50, 'gemm_f32_64x64': 3}},
 'one_block': {'f32': {'gemm_f32_256x32': 8, 'gemm_f32_64x64': 13},
               'bf16': {'convslab_bf16_128x128': 6,
                        'convslab_bf16_256x32': 7,
                        'convslab_bf16_256x64': 1,
                        'resfuse_bf16_c32': 2,
                        'resfuse_bf16_c64': 2}},
 'four_blocks': {'f32': {'gemm_f32_256x32': 48, 'gemm_f32_64x64': 28},
                 'bf16': {'convreg_bf16_c32': 6,
                          'convreg_bf16_c64': 6,
                          'convslab_bf16_128x128': 1,
                          'convslab_bf16_256x32': 32,
                          'convslab_bf16_256x64': 7,
                          'resstream_bf16_c32': 2,
                          'resstream_bf16_c64': 3}},
 'one_dilation': {'f32': {'gemm_f32_256x32': 8, 'gemm_f32_64x64': 8},
                  'bf16': {'convslab_bf16_128x128': 1,
                           'convslab_bf16_256x32': 6,
                           'convslab_bf16_256x64': 1,
                           'resfuse_bf16_c32': 2,
                           'resfuse_bf16_c64': 2}},
 'stream_tails': {'f32': {'gemm_f32_256x32': 12, 'gemm_f32_64x64': 10},
                  'bf16': {'convslab_bf16_128x128': 1,
                           'convslab_bf16_256x32': 8,
                           'convslab_bf16_256x64': 1,
                           'resfuse_bf16_c32': 3,
                           'resstream_bf16_c64': 2}},
 'rb2_three': {'f32': {'gemm_f32_256x32': 12, 'gemm_f32_64x64': 15},
               'bf16': {'convreg_bf16_c32': 9,
                        'convreg_bf16_c64': 9,
                        'convslab_bf16_128x128': 1,
                        'convslab_bf16_256x32': 5,
                        'convslab_bf16_256x64': 3}},
 'rb2_one': {'f32': {'gemm_f32_256x32': 4, 'gemm_f32_64x64': 3},
             'bf16': {'convreg_bf16_c32': 1, 'convslab_bf16_128x128': 1, 'convslab_bf16_256x32': 4, 'gemm_bf16_256x32': 1}},
 'odd_rates': {'f32': {'gemm_f32_256x32': 37, 'gemm_f32_64x64': 16},
               'bf16': {'convslab_bf16_256x32': 4,
                        'convslab_bf16_256x64': 1,
                        'narrowstage_c16': 1,
                        'narrowstage_c8': 1,
                        'resstream_bf16_c32': 2,
                        'resstream_bf16_c64': 3}}}


def runs(case, prec):
    r = SWEEP[case]["refused"]
    return r is None or prec not in r


def batch_lengths(case):
    pmax = SWEEP[case]["pmax"]
    return np.array([pmax, 1, pmax // 2], np.int32)


def batch_mel(case, seed=0, n_mels=80):
    """The ragged batch of a case: N(0, 1) rows up to P[b], NaN behind them (a masked row must never be read)."""
    P = batch_lengths(case)
    rng = np.random.default_rng(1000 + seed)
    mel = np.full((len(P), int(P.max()), n_mels), np.nan, np.float32)
    for b, p in enumerate(P):
        mel[b, :p] = rng.standard_normal((p, n_mels)).astype(np.float32)
    return mel, P
