"""CPU: the hipRTC specialisation of k_tick builds for gfx950 with its rank workgroups compiled in
(JitSchema::kLb, what a world without record ops gets) and compiled out (NFGPU_JIT_LB=0), within
the kernel's register budget either way.  Needs no GPU (nfk_jit_preview)."""
import pytest

from noahgameframe_amd import kernel, workload


@pytest.mark.parametrize("lb", ["1", "0"], ids=["rank-mode-on", "rank-mode-off"])
def test_rank_mode_policy_compiles_for_gfx950(monkeypatch, lb):
    monkeypatch.setenv("NFGPU_JIT_LB", lb)
    w = workload.make_world(n_obj=512, n_ticks=1)
    src, ok, msg = kernel.jit_preview(w, compile=True)
    assert ok, msg
    assert f"kLb = {'true' if lb == '1' else 'false'};" in src
    assert msg.startswith("_ZN5nfgpu6k_tick") and "JitSchema" in msg
    # the compiler's resource remarks, one "name: value" per line after each "Function Name:"
    usage, fn = {}, None
    for line in msg.splitlines():
        k, _, v = line.strip().partition(": ")
        if k == "Function Name":
            fn = v
            usage[fn] = {}
        elif fn is not None and v:
            usage[fn][k] = v
    tick = [f for f in usage if "k_tick" in f]
    assert len(tick) == 1, msg
    print(tick[0], usage[tick[0]])
    # the rank workgroups' code shares the kernel: it must not cost the tiles a register spill or
    # scratch, nor push the kernel past 5 waves per SIMD (at most 96 vector registers)
    assert int(usage[tick[0]]["VGPRs Spill"]) == 0, usage[tick[0]]
    assert int(usage[tick[0]]["ScratchSize [bytes/lane]"]) == 0, usage[tick[0]]
    assert int(usage[tick[0]]["VGPRs"]) <= 512 // 5 // 8 * 8
