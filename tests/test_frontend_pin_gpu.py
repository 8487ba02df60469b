"""The feature front end of fft.hip on its own, through the C ABI, against the float64 restatement of tests/frontend_ref.py:
trunet_stft_features / trunet_pcen, their frames-last and ragged siblings and the lockstep trunet_stream_features, at the
smallest shapes that reach their edges (tests/frontend_cases.py, where the cases and every tolerance are stated).  Every
element of every output is compared and no bin is masked out; outputs are prefilled with NaN, every buffer has a sentinel
behind it, and a repeat launch must give the same bits.  DESIGN.md, "What pins the feature front end", has the table of
what a run measured.  trunet_stream_features_rows and trunet_stream_feed_features / _commit are held bit for bit to the
offline path by tests/test_stream_pool_gpu.py and tests/test_stream_feed_gpu.py."""
import pytest
import torch

import frontend_cases as G

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("L", G.FEAT_L)
def test_stft_features_match_fp64(L):
    """trunet_stft_features (C = 3 and 4, with mag and with mag = NULL) and trunet_stft_features_fl (NP = 256 and 512) on
    three different utterances per case: Gaussian at 0.1 and 30, a tone on a bin centre, an impulse, a DC offset, 1e-9,
    exact zeros, and exactly silent frames on either side of a pair"""
    for case in G.FEAT_CASES:
        if case[0] == L:
            c = G.feat_inputs(case)
            got = G.feat_gpu(c)
            G.judge_feat(c, got)
            G.same_bits(got, G.feat_gpu(c), c.tag)


@pytest.mark.parametrize("case", G.FL_EDGE_CASES, ids=lambda k: "B%d-L%d" % k)
def test_frames_last_features_at_a_full_and_a_one_short_pad(case):
    """N = B T = 256 (NP = 256 has no spare column) and N = 255"""
    c = G.fl_edge_inputs(case)
    G.judge_feat(c, G.feat_gpu(c, fl=(256,)))


@pytest.mark.parametrize("C", (3, 4))
def test_ragged_features_match_fp64_and_the_dense_entry_point_bit_for_bit(C):
    for i in range(len(G.RAGGED_CASES)):
        c = G.ragged_inputs(i, C)
        got = G.ragged_gpu(c)
        G.judge_ragged(c, got)
        G.same_bits(got, G.ragged_gpu(c), c.tag)


@pytest.mark.parametrize("T", G.PCEN_T)
def test_pcen_matches_fp64(T):
    """trunet_pcen (out_stride 257 and 4 * 257) and trunet_pcen_fl on given magnitudes around the 256- and 128-frame chunks
    of their scans: generic, zeros then a burst, a burst then zeros, all zeros (exact zeros out), one value of 1e4"""
    for case in G.PCEN_CASES:
        if case[0] == T:
            c = G.pcen_inputs(case)
            got = G.pcen_gpu(c)
            G.judge_pcen(c, got)
            G.same_bits(got, G.pcen_gpu(c), c.tag)


def test_ragged_pcen_restarts_per_utterance():
    """three utterances of 3, 256 and 2 frames: the restart inside a chunk and on a chunk's edge; bit for bit the dense
    entry point on each utterance alone"""
    c = G.pcen_ragged_inputs()
    got = G.pcen_ragged_gpu(c)
    G.judge_pcen(c, got)
    G.same_bits(got, G.pcen_ragged_gpu(c), c.tag)


@pytest.mark.parametrize("S", G.STREAM_S)
def test_lockstep_stream_features_match_fp64(S):
    """trunet_stream_features: `first` with chunk NULL on a prefilled ring, then five hops; the ring is the exact shift, the
    channels and the carried smoother lie inside the float64 interval of the unexposed magnitude"""
    for case in G.STREAM_CASES:
        if case[0] == S:
            c = G.stream_inputs(case)
            got = G.stream_gpu(c)
            G.judge_stream(c, got)
            G.same_bits(got, G.stream_gpu(c), c.tag)


@pytest.mark.parametrize("L", G.SILENT_L)
def test_exactly_silent_frames_have_the_reference_values(L):
    """A frame whose 512 staged samples are exactly zero, next to a loud partner in the shared transform: mag == 0,
    nm == -1, (sin, cos) == (0, 1) and PCEN 0, as torch.stft has it, in the dense, frames-last and ragged entry points (the
    lockstep one: the `mute` cases of test_lockstep_stream_features_match_fp64).  Before the silent-frame guard of fft.hip
    the partner's rounding leaked in: max |X| 6.7e-7 and PCEN up to 0.17 at amplitude 0.5 (0.035 at 0.1) where the reference has
    0, and 0.34 in a muted lockstep stream beside one at 0.5 (DESIGN.md has the run)."""
    assert G.judge_silent(L, G.silent_gpu(L)) > 0
