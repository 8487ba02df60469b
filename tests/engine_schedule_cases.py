"""The cases of the launch-trace test (tests/test_engine_schedule_gpu.py) and of its recorder
(tests/golden/make_engine_launch_trace.py): one training step run directly on an engine with profiling on, reduced to the
ordered list of (kernel family, tag) of its profiled launches.  The kernel family is the recorded kernel name up to its
``<``: the template arguments mirror the library's dispatch, which a kernel change may move without touching the schedule."""
import os

import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_launch_trace.json")
N_FRAMES = 3           # NP = 256; divisible by the T = 3 of the TGRU case

# name -> (bf16 engine?, tgru_T, toggles set to False: (module name, attribute))
CASES = {
    "fp32": (False, None, []),
    "fp32_tgru": (False, 3, []),
    "bf16": (True, None, []),
    "fp32_unfused": (False, None, [("engine", "FUSED_PWBWD"), ("engine", "FUSED_CONVT"), ("engine", "FUSED_THIN"),
                                   ("engine", "FUSED_GRU_PROJ")]),
    "bf16_unfused": (True, None, [("engine_bf16", "FUSED_PWBWD16"), ("engine_bf16", "FUSED_CONVT16")]),
    # both: GRU_IO16 is computed from GRU_PROJ16 at import
    "bf16_gru_fp32": (True, None, [("engine_bf16", "GRU_PROJ16"), ("engine_bf16", "GRU_IO16")]),
    "bf16_last_ct_bf16": (True, None, [("engine_bf16", "LAST_CT32")]),
}


def run_case(name, setattr_, steps=1):
    """Traces of `steps` consecutive recorded training steps of case `name` on one engine.  setattr_(module, attribute,
    value) switches a toggle off and is responsible for putting it back (monkeypatch.setattr in the test)."""
    from tinyrecurrentunet_amd import engine, engine_bf16
    from tinyrecurrentunet_amd.network import TRUNet
    bf16, tgru_T, off = CASES[name]
    mods = {"engine": engine, "engine_bf16": engine_bf16}
    for mod, attr in off:
        assert getattr(mods[mod], attr) is True, "%s.%s is off in the environment" % (mod, attr)
        setattr_(mods[mod], attr, False)
    torch.manual_seed(0)
    # use_tgru with tgru_T: the TGRU parameters get their slots in the flat gradient buffer only then
    net = TRUNet(input_size=4, use_tgru=tgru_T is not None).cuda().train()
    eng = (engine_bf16.TRUNetEngineBF16 if bf16 else engine.TRUNetEngine)(net)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    x = torch.randn(N_FRAMES, 4, 257, generator=g, device="cuda")
    gout = torch.randn(N_FRAMES, 8, 257, generator=g, device="cuda")
    traces = []
    for _ in range(steps):
        old = engine.PROFILE, engine.PROFILE_LOG
        engine.PROFILE, engine.PROFILE_LOG = {}, []
        try:
            _, ctx = eng.forward(x, True, tgru_T=tgru_T, record=True)
            eng.backward(ctx, gout)
            torch.cuda.synchronize()
            traces.append([[rec[0].split("<")[0], rec[1]] for rec in engine.PROFILE_LOG])
        finally:
            engine.PROFILE, engine.PROFILE_LOG = old
    return traces
