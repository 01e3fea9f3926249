"""The documented order of enf_signal_sum (csrc/enf_loss.hip: sum256), emulated in numpy float32 -- what tests/test_gpu_loss_forms.py holds
the kernel to, bit for bit -- and the proof that the comparison can fail: on the test's own input a plain np.sum gives other bits."""
import numpy as np

SIGNAL_SUM_N = (1, 255, 256, 257, 1000)


def signal_sum_input(N, B=3):
    """err (B, N) float32 of mixed sign and magnitude (six decades), seeded by N."""
    rng = np.random.default_rng(1000 + N)
    return (rng.standard_normal((B, N)) * 10.0 ** rng.uniform(-3, 3, (B, N))).astype(np.float32)


def signal_sum_emulated(err, scale):
    """loss_b[b] = (sum of err[b]) * scale in the kernel's order: thread t of 256 adds err[b, t], err[b, t + 256], ... in order onto
    0.0f, then the tree red[t] += red[t + o] for o = 128, 64, ..., 1; every operation in float32."""
    B, N = err.shape
    red = np.zeros((B, 256), np.float32)
    for k in range(0, N, 256):
        chunk = err[:, k:k + 256]
        red[:, :chunk.shape[1]] += chunk
    o = 128
    while o > 0:
        red[:, :o] += red[:, o:2 * o]
        o >>= 1
    return red[:, 0] * np.float32(scale)


def test_emulation_is_the_plain_sum_up_to_rounding():
    for N in SIGNAL_SUM_N:
        err = signal_sum_input(N)
        ref = err.astype(np.float64).sum(1) / N
        got = signal_sum_emulated(err, 1.0 / N)
        # N additions of float32 values: at most N ulp of the sum of magnitudes
        assert np.all(np.abs(got - ref) <= N * 2.0 ** -23 * np.abs(err).astype(np.float64).sum(1) / N + 1e-30)


def test_emulation_differs_in_bits_from_np_sum():
    """Not every order gives these bits: where a thread adds more than one value (N = 1000) numpy's pairwise float32 sum differs from the
    emulation in at least one signal, so an order other than the documented one can be caught."""
    err = signal_sum_input(1000)
    plain = err.sum(1, dtype=np.float32) * np.float32(1.0 / 1000)
    assert not np.array_equal(plain.view(np.uint32), signal_sum_emulated(err, 1.0 / 1000).view(np.uint32))
    assert np.array_equal(signal_sum_emulated(err[:, :1], 1.0).view(np.uint32), err[:, 0].view(np.uint32))      # one value: itself
