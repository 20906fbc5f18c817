"""The designed-score generator of tests/test_gpu_attention_patterns.py, checked without a GPU:
its inputs are bf16-exact with fp32-exact scores, the tie pattern makes a double-counted key
visible, offset_big reaches the bf16-rounded-max hazard, and each pattern drives the
deferred-rescale rule the way it is meant to (emulated on the CPU)."""
from tests.test_gpu_attention_patterns import PATTERNS, ROWS, check_generator, make_case


def test_generator_invariants_hold():
    # one shape per padded head width and per tail kind: one key past a 32-block, a ragged
    # 64-chunk, the longest row, a dk that fills neither 64 nor 128
    check_generator([(20, 33), (64, 131), (64, 300), (100, 200)])


def test_every_kernel_row_gets_every_pattern():
    kernels = {r[0] for r in ROWS}
    assert kernels == {"f32", "bf16-4wave", "bf16-8wave", "bf16-persistent", "bf16-ps16",
                       "bf16-ldsdma", "bf16-generic", "bf16x3", "bf16x3-kc64"}
    assert {r[2] for r in ROWS if r[0] == "bf16-8wave"} == {-1, 2, 3}
    qkv, exp, extra, s = make_case(PATTERNS[0], 33, 20)
    assert qkv.shape == (2 * 33, 3 * 2 * 32 + 8) and exp.shape == (2, 33, 2, 20) and extra == 0.0
