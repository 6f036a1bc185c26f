"""The table of front-end shapes the sweep of test_frontend_shapes.py walks: phoneme encoder, variance adaptor, both mel decoders and the
speaker encoder at model configurations off config.medium_modelcfg / config.reduced_modelcfg, the only two every other test builds.

The routing layer of zvx.hip (read_config, fft_block, variance_predictor, run_encode, decoder_fs2, decoder_styletts, sty_conv / sty_norm,
spkemb_from_mels) turns ANY modelcfg into launches, and which kernels it launches follows from the widths: the fused attentions exist for
head depth 264 only, the FS2 decoder computes in IEEE half only there, the conv-GEMM tile and its compile-time epilogue follow from
N = H, 2H, 2H + 64, a StyleTTS block's 1x1 shortcut is a second source of its k = 3 convolution only where both K are multiples of 16,
and the speaker encoder's levels pick persistent, stride-2 or gathered-row kernels by channel count.

A case is a set of overrides on config.reduced_modelcfg(kind) (packed blobs of 2 ... 52 MB), packed with the smallest named generator
(config "tiny2", its conv_pre taking the case's num_mels).  The checker is the oracle; the fixtures tests/golden/sweep_<case>.npz (written by
tests/golden/gen_golden.py from the reference itself) pin the oracle at every shape of the table, the refused ones included.
"""
from __future__ import annotations

import copy
import zlib

import numpy as np

from zerovox_amd import config as zcfg

VOC = "tiny2"                                             # the generator every case is packed with (never run: the vocoder is not under test)
T_ROWS = (13, 1, 7)                                       # phonemes per utterance of the ragged batch: padding, a one-row utterance
REF_FRAMES = (97, 33, 258)                                # reference mels: odd widths at every level; 258 frames = a second 64-position tile

# ------------------------------------------------------------------------------------------------------------------------------
# The sweep.  Keys of an entry (all but `kind` optional; what is absent keeps reduced_modelcfg's value):
#   kind            decoder kind
#   emb             emb_dim (punct_emb_dim stays 16: hidden = emb + 16)
#   heads           (encoder fs2_head, decoder n_head)
#   ffn, ffn_k      decoder conv_filter_size / conv_kernel_size (the encoder's FFN uses them too, model.py:211-212)
#   vp, vp_k, bins  encoder vp_filter_size / vp_kernel_size / ve_n_bins
#   scln, layers    decoder scln; (encoder fs2_layer, decoder n_layers)
#   mels            audio num_mels
#   rn_filters, rn_layers, pool     resnet num_filters / layers / encoder_type
#   max_txt, max_mel                max_txt_len / max_mel_len (rows of the stored position tables)
#   voc_mels        input channels of the generator's conv_pre where they differ from num_mels
#   seed            added to crc32(name): the data seed, picked so that the oracle's discrete decisions sit off their rounding boundaries
#   refused         None: runs.  Otherwise {precision: (modelcfg field, manifest key, zvx status name)} the refusal has to name -- at
#                   pack_model and at zvx_create ("ENCODE": zvx_create accepts the manifest, the first zvx_encode refuses)
#   fixture         False: the reference itself cannot run the config, so no sweep_<case>.npz exists (why: beside the entry)
#   dec16           the arithmetic of the mel decoder in the 16-bit context: "f16" (check_mel's half limits) or "bf16" (its kind "bf16")
# ------------------------------------------------------------------------------------------------------------------------------
_BOTH = lambda field, key, status="UNSUPPORTED": {"f32": (field, key, status), "bf16": (field, key, status)}  # noqa: E731

SWEEP = {
    # head depth 264 at H = 264 (one head): the fused f32 attention in the encoder, the flash attention and the IEEE-half FS2 decoder with
    # ldq = 2H / 3H = 528 / 792 instead of 1056 / 1584; K = 264 is no multiple of 16: every 16-bit GEMM on the gathered-row kernel
    "h264_1head_fs2": dict(kind="fastspeech2", emb=248, heads=(1, 1), dec16="f16"),
    # head depth 176 at the medium width (4 heads would be depth 132: refused, no multiple of 8): unfused QK / softmax / PV in f32 and in
    # bf16; decoder_fs2 must fall to bf16; the encoder's split-plane products (3H a multiple of 16) with the three-launch attention
    "h528_3head_fs2": dict(kind="fastspeech2", emb=512, heads=(3, 3), dec16="bf16"),
    # CW = 2H + 64 = 592; the encoder fused; the StyleTTS decoder in half with K = 264 / 528 / 592
    "h264_sty": dict(kind="styletts", emb=248, heads=(1, 1), dec16="f16"),
    # 2H = 128: the 128-wide tiles' compile-time epilogues and the shortcut fused as a second source (K2) at N = 128 and N = 64 (medium
    # never has N = 128 there); speaker encoder: a stride-2 level with Cin = Cout (64 -> 64), one that narrows (64 -> 32), two blocks in
    # the first and the last level
    "h64_sty": dict(kind="styletts", emb=48, rn_filters=[32, 64, 64, 32], rn_layers=[2, 1, 1, 2], dec16="f16"),
    # H = 128, 2H = 256, CW = 320; mel projection N = 64; the pooled map has Fp = 8 frequency rows; a 16-channel first level
    "h128_sty_mels64": dict(kind="styletts", emb=112, mels=64, rn_filters=[16, 32, 64, 128], rn_layers=[1, 2, 1, 1], dec16="f16"),
    # no width a multiple of 64 (136, 272, 336), H none of 16: partial N tiles, partial K chunks, two shortcuts as their own launches; a k = 3
    # second FFN convolution; 17 bins; vp 40, FFN 72 (multiples of 8 only); one head of depth 136
    "h136_sty_k53": dict(kind="styletts", emb=120, heads=(1, 1), ffn=72, ffn_k=[5, 3], vp=40, bins=17, dec16="f16"),
    # plain-LayerNorm decoder blocks (ln1_g / ln2_g, no dec.scln_all GEMM); single-layer stacks; both FFN kernels 3 (batch-flattened halo 1)
    "h64_noscln_fs2": dict(kind="fastspeech2", emb=48, scln=False, layers=(1, 1), ffn_k=[3, 3], dec16="bf16"),
    # H = 40 (one encoder head of depth 40; five decoder heads of depth 8); 40 mels: Fp = 5 (odd), mel projection N = 40; SAP pooling
    "h40_mels40_sap": dict(kind="fastspeech2", emb=24, heads=(1, 5), mels=40, pool="SAP", rn_filters=[32, 32, 64, 64], dec16="bf16"),
    # stored position tables of 8 / 16 rows: both recomputed (T = 13 > 8, L > 16); differing head counts (depth 16 / 64); n_bins - 1 = 1
    "bins2_txt8": dict(kind="fastspeech2", emb=48, heads=(4, 1), bins=2, max_txt=8, max_mel=16, dec16="bf16"),
    # head depth 24 (three heads); H = 72 is no multiple of 16: the shortcuts of encode.0 and decode.2 run as their own launches
    "h72_3head": dict(kind="styletts", emb=56, heads=(3, 3), dec16="f16"),
    # the largest odd tap count a convolution launch takes (16 taps); batch-flattened halo 7
    "k15_k1": dict(kind="fastspeech2", emb=48, ffn_k=[15, 1], dec16="bf16"),
    # H = 64 gives the encoder's projections split planes (3H a multiple of 16), FFN 72 leaves its second convolution without (3 x 72 = 216):
    # the block must run all four static-weight GEMMs on the exact-f32 MFMA, not look for planes that were never built
    "h64_ffn72": dict(kind="fastspeech2", emb=48, ffn=72, dec16="bf16"),
    # FFN width 68: four floats per group in f32 (runs), no multiple of the 8-element groups of the 16-bit kernels (refused)
    "ffn68": dict(kind="fastspeech2", emb=48, ffn=68, dec16="bf16", refused={"bf16": ("conv_filter_size", "ffn_dim", "UNSUPPORTED")}),
    # ---- refused in both precisions ----
    # hidden 36: no multiple of 8
    "h36": dict(kind="styletts", emb=20, refused=_BOTH("emb_dim", "hidden")),
    # three heads do not divide hidden 40.  No fixture: the reference floors the depth to 13 and projects Q / K / V to 39 columns
    # (fs2.py:118-120), a shape neither weights.tts_state_dict nor the oracle models
    "h40_3head": dict(kind="styletts", emb=24, heads=(3, 2), refused=_BOTH("fs2_head", "enc_heads"), fixture=False),
    # 17 taps: one more than a convolution launch carries
    "k17_k1": dict(kind="fastspeech2", emb=48, ffn_k=[17, 1], refused=_BOTH("conv_kernel_size", "ffn_k")),
    # the variance predictors' bias and stores go in groups of four floats
    "vp42": dict(kind="styletts", emb=48, vp=42, refused=_BOTH("vp_filter_size", "vp_dim")),
    # a generator whose conv_pre takes 80 channels under a 40-mel model: the manifest contradicts its own tensors
    "voc80_mels40": dict(kind="styletts", emb=48, mels=40, voc_mels=80, refused=_BOTH("num_mels", "n_mels", "MANIFEST")),
    # 44 mels: no multiple of 8.  No fixture: the reference cannot build it (ResNetSE34V2.py:128 sizes the attention for
    # int(44 / 8) = 5 frequency rows, three stride-2 levels leave 6)
    "mels44": dict(kind="styletts", emb=48, mels=44, refused=_BOTH("num_mels", "n_mels"), fixture=False),
    # vp_kernel_size 5: fs2.py:543 pads the second convolution with the literal 1, the prediction comes out two positions short.  Refused by
    # the first zvx_encode, as before this table existed.  No fixture: the reference fails adding the pitch embedding (T - 2 rows to T)
    "vp_k5": dict(kind="styletts", emb=48, vp_k=5, refused=_BOTH("vp_kernel_size", "vp_k", "ENCODE"), fixture=False),
}

# ROUTING: what zvx_kernel_stats must and must not show for ONE encode + decode of the ragged batch (forced durations), every fusion on.
#   present / absent   kernel-name prefixes per precision
#   sc_fused           StyleTTS only: launches the call saves against zvx_set_int("dec_sc_fuse", 0) -- 4 where the shortcuts of encode.0 and
#                      decode.0-2 all run inside the k = 3 convolution; 2 where H is no multiple of 16: decode.0 / .1 (K = 2H, K2 = 2H + 64)
#                      still fuse, encode.0 (K = K2 = H) and decode.2 (K = H) run the shortcut as its own launch
# LAUNCHES (below): per case and precision the launch count per kernel name of that call ("front") and of ONE zvx_spkemb call on the three
# ragged reference mels ("spk"), as recorded on the MI355X (profiles/frontend_shape_sweep.txt): a routing change has to edit it knowingly.
_FUSED = dict(present={"f32": ("attention_f32",), "bf16": ("attention_f32",)})
_UNFUSED = dict(absent={"f32": ("attention_f32", "flash_attention"), "bf16": ("attention_f32", "flash_attention")})
ROUTING = {
    "h264_1head_fs2": dict(present={"f32": ("attention_f32",), "bf16": ("attention_f32", "flash_attention_f16")}, absent={"f32": ("flash_attention",), "bf16": ("flash_attention_bf16",)}),
    "h528_3head_fs2": _UNFUSED,
    "h264_sty": dict(_FUSED, absent={"f32": ("flash_attention",), "bf16": ("flash_attention",)}, sc_fused=2),
    "h64_sty": dict(_UNFUSED, sc_fused=4),
    "h128_sty_mels64": dict(_UNFUSED, sc_fused=4),
    "h136_sty_k53": dict(_UNFUSED, sc_fused=2),
    "h64_noscln_fs2": _UNFUSED,
    "h40_mels40_sap": _UNFUSED,
    "bins2_txt8": _UNFUSED,
    "h72_3head": dict(_UNFUSED, sc_fused=2),
    "k15_k1": _UNFUSED,
    "h64_ffn72": _UNFUSED,
    "ffn68": _UNFUSED,
}

LAUNCHES = {'h264_1head_fs2': {'f32': {'front': {'attention_f32': 4, 'gemm_f32_256x32': 6, 'gemm_f32_64x64': 18},
                            'spk': {'gemm_f32_256x32': 11, 'gemm_f32_64x64': 2}},
                    'bf16': {'front': {'attention_f32': 2,
                                       'convslab_bf16_256x32': 2,
                                       'flash_attention_f16': 2,
                                       'gemm_bf16_64x64': 7,
                                       'gemm_f32_256x32': 6,
                                       'gemm_f32_64x64': 9},
                             'spk': {'convslab_bf16_256x32': 1, 'gemm_bf16_256x32': 11, 'gemm_bf16_64x64': 1}}},
 'h528_3head_fs2': {'f32': {'front': {'gemm_f32_256x32': 14, 'gemm_f32_64x64': 22}, 'spk': {'gemm_f32_256x32': 11, 'gemm_f32_64x64': 2}},
                    'bf16': {'front': {'convslab_bf16_256x32': 17,
                                       'gemm_bf16_256x32': 4,
                                       'gemm_bf16_64x64': 2,
                                       'gemm_f32_256x32': 10,
                                       'gemm_f32_64x64': 3},
                             'spk': {'convslab_bf16_256x32': 1, 'gemm_bf16_256x32': 11, 'gemm_bf16_64x64': 1}}},
 'h264_sty': {'f32': {'front': {'attention_f32': 2, 'gemm_f32_256x32': 6, 'gemm_f32_64x64': 29}, 'spk': {'gemm_f32_256x32': 11, 'gemm_f32_64x64': 2}},
              'bf16': {'front': {'attention_f32': 2, 'convslab_bf16_256x32': 8, 'gemm_bf16_64x64': 10, 'gemm_f32_256x32': 6, 'gemm_f32_64x64': 9},
                       'spk': {'convslab_bf16_256x32': 1, 'gemm_bf16_256x32': 11, 'gemm_bf16_64x64': 1}}},
 'h64_sty': {'f32': {'front': {'gemm_f32_256x32': 12, 'gemm_f32_64x64': 29}, 'spk': {'gemm_f32_256x32': 9, 'gemm_f32_64x64': 8}},
             'bf16': {'front': {'convreg_bf16_c64': 5, 'convslab_bf16_256x32': 19, 'gemm_f32_256x32': 12, 'gemm_f32_64x64': 1},
                      'spk': {'conv2d_persist_c32': 4,
                              'conv2d_persist_c64': 2,
                              'conv2d_s2_c32': 1,
                              'convreg_bf16_c32': 3,
                              'convslab_bf16_256x32': 1,
                              'gemm_bf16_256x32': 2,
                              'gemm_bf16_64x64': 3}}},
 'h128_sty_mels64': {'f32': {'front': {'gemm_f32_256x32': 10, 'gemm_f32_64x64': 31}, 'spk': {'gemm_f32_256x32': 7, 'gemm_f32_64x64': 8}},
                     'bf16': {'front': {'convslab_bf16_256x32': 24, 'gemm_f32_256x32': 10, 'gemm_f32_64x64': 3},
                              'spk': {'conv2d_persist_c32': 3,
                                      'conv2d_persist_c64': 1,
                                      'conv2d_s2_c32': 1,
                                      'conv2d_s2_c64': 1,
                                      'convslab_bf16_128x128': 1,
                                      'convslab_bf16_256x32': 1,
                                      'gemm_bf16_256x32': 4,
                                      'gemm_bf16_64x64': 2}}},
 'h136_sty_k53': {'f32': {'front': {'gemm_f32_256x32': 4, 'gemm_f32_256x64': 6, 'gemm_f32_64x64': 31},
                          'spk': {'gemm_f32_256x32': 11, 'gemm_f32_64x64': 2}},
                  'bf16': {'front': {'convslab_bf16_256x32': 8,
                                     'gemm_bf16_64x64': 10,
                                     'gemm_f32_256x32': 4,
                                     'gemm_f32_256x64': 6,
                                     'gemm_f32_64x64': 11},
                           'spk': {'convslab_bf16_256x32': 1, 'gemm_bf16_256x32': 11, 'gemm_bf16_64x64': 1}}},
 'h64_noscln_fs2': {'f32': {'front': {'gemm_f32_256x32': 12, 'gemm_f32_64x64': 9}, 'spk': {'gemm_f32_256x32': 11, 'gemm_f32_64x64': 2}},
                    'bf16': {'front': {'convreg_bf16_c64': 2, 'convslab_bf16_256x32': 7, 'gemm_bf16_256x32': 3, 'gemm_f32_256x32': 9},
                             'spk': {'convslab_bf16_256x32': 1, 'gemm_bf16_256x32': 11, 'gemm_bf16_64x64': 1}}},
 'h40_mels40_sap': {'f32': {'front': {'gemm_f32_256x32': 12, 'gemm_f32_256x64': 15, 'gemm_f32_64x64': 9},
                            'spk': {'gemm_f32_256x32': 5, 'gemm_f32_64x64': 8}},
                    'bf16': {'front': {'convslab_bf16_256x64': 2,
                                       'gemm_bf16_256x32': 2,
                                       'gemm_bf16_256x64': 7,
                                       'gemm_bf16_64x64': 4,
                                       'gemm_f32_256x32': 10,
                                       'gemm_f32_256x64': 6,
                                       'gemm_f32_64x64': 5},
                             'spk': {'conv2d_persist_c32': 3,
                                     'conv2d_persist_c64': 1,
                                     'conv2d_s2_c32': 1,
                                     'convreg_bf16_c64': 1,
                                     'convslab_bf16_256x32': 1,
                                     'gemm_bf16_256x32': 2,
                                     'gemm_bf16_64x64': 3}}},
 'bins2_txt8': {'f32': {'front': {'gemm_f32_256x32': 16, 'gemm_f32_64x64': 20}, 'spk': {'gemm_f32_256x32': 11, 'gemm_f32_64x64': 2}},
                'bf16': {'front': {'convslab_bf16_256x32': 17,
                                   'gemm_bf16_256x32': 4,
                                   'gemm_bf16_64x64': 2,
                                   'gemm_f32_256x32': 12,
                                   'gemm_f32_64x64': 1},
                         'spk': {'convslab_bf16_256x32': 1, 'gemm_bf16_256x32': 11, 'gemm_bf16_64x64': 1}}},
 'h72_3head': {'f32': {'front': {'gemm_f32_256x32': 12, 'gemm_f32_64x64': 29}, 'spk': {'gemm_f32_256x32': 11, 'gemm_f32_64x64': 2}},
               'bf16': {'front': {'convslab_bf16_256x32': 8, 'gemm_bf16_64x64': 10, 'gemm_f32_256x32': 12, 'gemm_f32_64x64': 9},
                        'spk': {'convslab_bf16_256x32': 1, 'gemm_bf16_256x32': 11, 'gemm_bf16_64x64': 1}}},
 'k15_k1': {'f32': {'front': {'gemm_f32_256x32': 18, 'gemm_f32_64x64': 18}, 'spk': {'gemm_f32_256x32': 11, 'gemm_f32_64x64': 2}},
            'bf16': {'front': {'convslab_bf16_256x32': 17, 'gemm_bf16_256x32': 6, 'gemm_f32_256x32': 12, 'gemm_f32_64x64': 1},
                     'spk': {'convslab_bf16_256x32': 1, 'gemm_bf16_256x32': 11, 'gemm_bf16_64x64': 1}}},
 'h64_ffn72': {'f32': {'front': {'gemm_f32_256x32': 18, 'gemm_f32_64x64': 18}, 'spk': {'gemm_f32_256x32': 11, 'gemm_f32_64x64': 2}},
               'bf16': {'front': {'convslab_bf16_256x32': 7, 'gemm_bf16_256x32': 6, 'gemm_bf16_64x64': 2, 'gemm_f32_256x32': 12, 'gemm_f32_64x64': 9},
                        'spk': {'convslab_bf16_256x32': 1, 'gemm_bf16_256x32': 11, 'gemm_bf16_64x64': 1}}},
 'ffn68': {'f32': {'front': {'gemm_f32_256x32': 18, 'gemm_f32_64x64': 18}, 'spk': {'gemm_f32_256x32': 11, 'gemm_f32_64x64': 2}}}}


def runs(case, prec):
    """True: the case runs in that precision and is held to parity.  False: refused, SWEEP[case]["refused"][prec] names the field."""
    r = SWEEP[case].get("refused")
    return r is None or prec not in r


def has_fixture(case):
    return SWEEP[case].get("fixture", True)


def modelcfg(case):
    e = SWEEP[case]
    cfg = zcfg.reduced_modelcfg(e["kind"])
    m = cfg["model"]
    if "emb" in e:
        m["emb_dim"] = e["emb"]
    if "heads" in e:
        m["encoder"]["fs2_head"], m["decoder"]["n_head"] = e["heads"]
    if "layers" in e:
        m["encoder"]["fs2_layer"], m["decoder"]["n_layers"] = e["layers"]
    for key, (sec, field) in (("ffn", ("decoder", "conv_filter_size")), ("ffn_k", ("decoder", "conv_kernel_size")), ("scln", ("decoder", "scln")),
                              ("vp", ("encoder", "vp_filter_size")), ("vp_k", ("encoder", "vp_kernel_size")), ("bins", ("encoder", "ve_n_bins")),
                              ("rn_filters", ("resnet", "num_filters")), ("rn_layers", ("resnet", "layers")), ("pool", ("resnet", "encoder_type"))):
        if key in e:
            m[sec][field] = copy.deepcopy(e[key])
    if "max_txt" in e:
        m["max_txt_len"] = e["max_txt"]
    if "max_mel" in e:
        m["max_mel_len"] = e["max_mel"]
    if "mels" in e:
        cfg["audio"]["num_mels"] = e["mels"]
    return cfg


def hidden(case):
    m = modelcfg(case)["model"]
    return m["emb_dim"] + m["punct_emb_dim"]


def voc_mels(case):
    return SWEEP[case].get("voc_mels", modelcfg(case)["audio"]["num_mels"])


def inputs(case):
    """The seeded inputs of a case: a ragged batch of three utterances (ids 0 behind an utterance's end), forced durations in [0, 5) with one
    zero and one 9 in the rows long enough to hold both (L < 60 frames), unit-norm style vectors, and three reference mels (N(0, 1),
    NaN behind a clip's end: a masked frame must never be read).  The one-phoneme utterance lasts ONE frame: repeated over 2 ... 5 frames
    its rows are identical, the StyleTTS decoder's InstanceNorm divides by a variance of ~0 and the reference's own f32 result is noise
    (test_gpu_parity.test_tiny_utterances: f32 against f64 differs by 2.0 at L = 2); one frame normalises to exactly zero everywhere."""
    rng = np.random.default_rng(zlib.crc32(case.encode()) + SWEEP[case].get("seed", 0))
    B, Tmax, H = len(T_ROWS), max(T_ROWS), hidden(case)
    n_mels = modelcfg(case)["audio"]["num_mels"]
    ph = np.zeros((B, Tmax), np.int32); pu = np.zeros((B, Tmax), np.int32); dur = np.zeros((B, Tmax), np.int32)
    for b, T in enumerate(T_ROWS):
        ph[b, :T] = rng.integers(1, len(zcfg.PHONES) + 1, T)
        pu[b, :T] = rng.integers(0, len(zcfg.PUNCTS) + 2, T)
        dur[b, :T] = rng.integers(0, 5, T)
        if T >= 3:
            dur[b, T // 3], dur[b, 2 * T // 3] = 0, 9
        else:
            dur[b, :T] = 1                                    # see the docstring
    spk = rng.standard_normal((B, H))
    spk = (spk / np.linalg.norm(spk, axis=1, keepdims=True)).astype(np.float32)
    lens = np.array(REF_FRAMES, np.int32)
    mels = np.full((len(lens), int(lens.max()), n_mels), np.nan, np.float32)
    for b, n in enumerate(lens):
        mels[b, :n] = rng.standard_normal((n, n_mels)).astype(np.float32)
    return dict(phoneme=ph, puncts=pu, T=np.array(T_ROWS, np.int32), duration=dur, spk=spk, ref_mels=mels, ref_lens=lens)
