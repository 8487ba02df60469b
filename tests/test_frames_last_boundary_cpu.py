"""Host-side argument checks of the frames-last boundary entry points of fft.hip (no GPU: nothing is launched)."""


def test_frames_last_entry_points_refuse_before_they_launch():
    """trunet_stft_features_fl / trunet_pcen_fl / trunet_mask_istft_fwd_fl / trunet_mask_istft_bwd_fl refuse what their
    siblings refuse, and a frame dimension that is not the layer kernels' (NP a positive multiple of 256, B T <= NP) --
    dummy non-null pointers are safe, nothing is launched."""
    from tinyrecurrentunet_amd import _lib
    lib = _lib.lib()
    EINVAL = _lib.TRUNET_EINVAL
    P = 0x1000

    def feat(B=3, L=512, T=5, C=4, NP=256, a=(P, P, P, P)):
        return lib.trunet_stft_features_fl(*a, B, L, T, C, NP, None)

    def pcen(B=3, T=5, NP=256, a=(P, P)):
        return lib.trunet_pcen_fl(*a, B, T, NP, 1e-6, 0.025, 0.98, 2.0, 0.5, None)

    def mfwd(B=3, T=5, L=512, NP=256, a=(P, P, P, P, P, P)):
        return lib.trunet_mask_istft_fwd_fl(*a, B, T, L, NP, 0.5, None)

    def mbwd(B=3, T=5, L=512, NP=256, a=(P, P, P, P)):
        return lib.trunet_mask_istft_bwd_fl(*a, B, T, L, NP, 0.5, None)

    for f in (feat, pcen, mfwd, mbwd):
        assert f(NP=0) == EINVAL and f(NP=-256) == EINVAL and f(NP=255) == EINVAL and f(NP=384) == EINVAL, f.__name__
        assert f(B=52) == EINVAL, f.__name__                       # 52 * 5 = 260 frames > NP = 256
        assert f(B=0) == EINVAL and f(B=-1) == EINVAL, f.__name__
    assert pcen(B=65536, T=65536, NP=256) == EINVAL                # B T past 2^31 does not wrap into a small N
    # the siblings' own checks
    assert feat(L=256) == EINVAL and feat(T=6) == EINVAL and feat(C=2) == EINVAL and feat(C=5) == EINVAL
    assert pcen(T=0) == EINVAL
    for f in (mfwd, mbwd):
        assert f(T=1, L=0) == EINVAL and f(L=511) == EINVAL and f(L=640) == EINVAL and f(T=6) == EINVAL
    for k in (0, 1, 3):                                            # mag (2) is optional
        a = [P, P, P, P]
        a[k] = None
        assert feat(a=tuple(a)) == EINVAL, k
    assert pcen(a=(None, P)) == EINVAL and pcen(a=(P, None)) == EINVAL
    for k in (0, 1, 2, 5):                                         # clean (3) and the L1 partials (4) are optional
        a = [P] * 6
        a[k] = None
        assert mfwd(a=tuple(a)) == EINVAL, k
    for k in range(4):
        a = [P] * 4
        a[k] = None
        assert mbwd(a=tuple(a)) == EINVAL, k
