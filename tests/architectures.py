"""Network architectures beside the reference's, shared by the CPU check of the float64 oracle (tests/test_oracle_dqn.py) and the GPU tests of the
per-layer implicit-GEMM path (tests/test_arch_gpu.py).  Plain module (test infrastructure), no fixtures.

dq_qnet_create accepts 1..4 convolutions, 0..4 hidden dense layers, any filter count and kernel size, a stride on the first convolution, any dropout
rate and up to 1024 actions; the fused chains cover the reference's stack only, everything else runs on csrc/qnet.hip + csrc/gemm.h.  Each entry below
is there for the forms of those kernels it reaches (GEMM view of a layer: M = batch * output pixels, N = filters / units, K = k * k * C_in / inputs):

  one_conv_no_hidden  n_ff = 0, a non-square input, K = 27 < 32 (one ragged K tile), N = 5, weight-gradient slice counts of 7 and 1
  k1_s1_two_hidden    K = 4, N = 33 and 48 (the N > 32 kernels with a ragged last column tile), two hidden layers (one with dropout), the dueling
                      kernels' loops at 65 > 64 actions, 13 and 18 weight-gradient slices
  four_convs          n_conv = 4, a first stride of 3, N = 70 (two column tiles, the second ragged), a dueling head over ONE action
  k5_s1_four_hidden   n_ff = 4, three dropout layers of different rates (ordinals 0, 1, 2 of the dropout draw), A + 1 = 130
  ref_hidden256       the reference's convolutions with a hidden width the fused chains refuse
  ref_cin11           the reference's stack on 11 input planes: K = 99 > 96, the first plane count past the fused chains
  big_rows            the 4-wave gemm_fwd_kernel<32, 4> and <64, 4> with ragged M (43 200 and 36 300 rows), 675 and 568 slices through
                      reduce_partials_kernel's 16-unrolled loop, a 4840-wide Flatten, 200 actions without a dueling head

The wide entries are the reference's stack on the observations and actions of d = 11, 13 and 15 (tests/test_env_wide_gpu.py CONFIGS): what DQNAgent.fit
creates there.  All of them run gemm_fwd_kernel<64, 1> / <32, 1> (at most 85 row tiles: far from the 256 blocks of the 4-wave forms) with a ragged last
row tile in every convolution, more than one row tile per sample (so the batch of one and the ring gather span 3 to 8 blocks), one weight-gradient slice
per dense layer (reduce_partials_kernel's tail loop alone, over up to 2.77 M elements) and a dueling head of 4 to 11 column tiles:

  wide_d11_dpy        23 x 23 x 7 input; Flatten 2592: 81 K tiles forward, gemm_wgrad_kernel<64> on a (21, 1, 8) grid whose last K block holds 32 of 128
                      rows, its data gradient over 41 column tiles (the last half full); head of 365 columns: 6 column tiles (45 in the last), K = 364 /
                      365 (12 K tiles, 12 and 13 in the last), the dueling kernels' loops 6 times with 44 lanes in the last pass
  wide_d13_dp         27 x 27 x 6 input, batch 7 (every dense row tile holds 7 of 32 rows); Flatten 3872: 121 K tiles, weight gradient on (31, 1, 8), data
                      gradient over 61 column tiles; head of 340 columns: K = 339 / 340 (19 and 20 in the last K tile), 19 and 20 columns in the last tile
  wide_d15_x          31 x 31 x 4 input (K = 36 in the first convolution, 85 / 74 / 64 row tiles, 43 / 37 / 32 weight-gradient slices); Flatten 5408: 169 K
                      tiles, weight gradient on (43, 1, 8), data gradient over 85 column tiles; head of 227 columns: 4 column tiles, K = 226 / 227
  wide_d15_dpy        the largest network the product creates (3.59 M parameters): the 5408-wide Flatten again, and a head of 677 columns: 11 column tiles
                      forward and as grid z of the weight gradient, whose (6, 1, 11) grid has a ragged last K block (36 of 128) AND a ragged last column
                      tile (37 of 64); K = 676 / 677: 22 K tiles (4 and 5 in the last); the dueling kernels' loops 11 times with 36 lanes in the last pass
"""
import numpy as np

from oracle import dqn_oracle as O

REF_CONV, REF_FF = [[64, 3, 2], [32, 2, 1], [32, 2, 1]], [[512, 0.2]]

# name -> (input_shape, c_layers, ff_layers, n_actions, dueling, batch)
ARCHITECTURES = {
    "one_conv_no_hidden": ((3, 9, 7), [[5, 3, 2]], [], 7, False, 33),
    "k1_s1_two_hidden": ((4, 6, 6), [[33, 1, 1], [48, 2, 1]], [[40, 0.5], [7, 0.0]], 65, True, 31),
    "four_convs": ((2, 13, 13), [[16, 4, 3], [70, 2, 1], [8, 2, 1], [32, 1, 1]], [[100, 0.2]], 1, True, 37),
    "k5_s1_four_hidden": ((1, 7, 9), [[24, 5, 1]], [[33, 0.3], [64, 0.0], [65, 0.1], [31, 0.6]], 129, True, 130),
    "ref_hidden256": ((7, 11, 11), REF_CONV, [[256, 0.2]], 51, True, 45),
    "ref_cin11": ((11, 11, 11), REF_CONV, REF_FF, 51, True, 45),
    "big_rows": ((3, 13, 13), [[8, 2, 1], [40, 2, 1]], [[16, 0.0]], 200, False, 300),
    # the observations and actions of four wide configurations of tests/test_env_wide_gpu.py (d11dpy, d13dp, d15x, d15dpy)
    "wide_d11_dpy": ((7, 23, 23), REF_CONV, REF_FF, 364, True, 11),
    "wide_d13_dp": ((6, 27, 27), REF_CONV, REF_FF, 339, True, 7),
    "wide_d15_x": ((4, 31, 31), REF_CONV, REF_FF, 226, True, 12),
    "wide_d15_dpy": ((6, 31, 31), REF_CONV, REF_FF, 676, True, 9),
}

# Seed of each entry's weight perturbation and observations (make_inputs): the first one from 5 upwards -- 5 is what tests/test_qnet_gpu.py's _setup
# uses -- for which NO sample has a ReLU pre-activation within 1e-6 of 0 in the training forward under DROPOUT's masks (oracle/dqn_oracle.py
# fragile_samples), so that every sample's gradient is compared with the float64 oracle as it stands.  big_rows has none among the first 55 seeds (300
# samples x 5992 ReLU units): it keeps seed 5 and its FRAGILE[name] = 3 such samples are compared under the side of each near-zero ReLU that the device
# took (tests/relu_choices.py).  The tests assert these counts; they do not rely on this table being right.
INPUT_SEED = {"one_conv_no_hidden": 5, "k1_s1_two_hidden": 5, "four_convs": 6, "k5_s1_four_hidden": 9, "ref_hidden256": 5, "ref_cin11": 5, "big_rows": 5,
              "wide_d11_dpy": 6, "wide_d13_dp": 5, "wide_d15_x": 9, "wide_d15_dpy": 5}
FRAGILE = {"one_conv_no_hidden": 0, "k1_s1_two_hidden": 0, "four_convs": 0, "k5_s1_four_hidden": 0, "ref_hidden256": 0, "ref_cin11": 0, "big_rows": 3,
           "wide_d11_dpy": 0, "wide_d13_dp": 0, "wide_d15_x": 0, "wide_d15_dpy": 0}

INIT_SEED = (11, 22)                        # glorot_init
DROPOUT = dict(seed=(3, 4), t=12345678901, sample_base=77)


def spec_of(name):
    shape, c_layers, ff_layers, A, dueling, _ = ARCHITECTURES[name]
    return O.QNetSpec(shape, c_layers, ff_layers, A, dueling=dueling)


def keep_masks(spec, batch, seed, t, sample_base):
    """One oracle keep mask per hidden layer with a dropout rate > 0, each drawn under its own ordinal (dqn_oracle.dropout_keep_mask layer=)."""
    rated = [(u, r) for u, r in spec.ff_layers if r > 0.0]
    return [O.dropout_keep_mask(seed, t, sample_base + np.arange(batch), u, r, layer=i) for i, (u, r) in enumerate(rated)]


def make_inputs(spec, batch, input_seed, init_seed=INIT_SEED):
    """(flat float32 parameters, uint8 observations, the RandomState behind them): Keras' initialisation plus N(0, 0.02) on every element -- non-zero
    biases, less symmetric weights -- and observations with 30 % of the cells set, as tests/test_qnet_gpu.py's _setup draws them."""
    rng = np.random.RandomState(input_seed)
    flat = O.glorot_init(spec, init_seed)
    flat = flat + (rng.randn(flat.size) * 0.02).astype(np.float32)
    obs = (rng.rand(batch, *spec.input_shape) < 0.3).astype(np.uint8)
    return flat, obs, rng


def entry(name):
    """(spec, batch, flat, obs, rng, keep masks of the training forward under DROPOUT) of an ARCHITECTURES entry."""
    spec, batch = spec_of(name), ARCHITECTURES[name][5]
    flat, obs, rng = make_inputs(spec, batch, INPUT_SEED[name])
    return spec, batch, flat, obs, rng, keep_masks(spec, batch, **DROPOUT)
