"""Training-for-guidance surface that needs no GPU: the two C prototypes as the ctypes binding parses them, and the
Trainer's keyword arguments and methods."""
import ctypes
import inspect


def test_header_declares_adam_ema_and_context_drop():
    from cdm_amd import _lib
    protos = _lib.parse_header()
    vp, i, ll, ull, ui, f, d = (ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_uint,
                                ctypes.c_float, ctypes.c_double)
    # p, g, m, v, ema, n, state, bc, nbc, beta1, beta2, eps, grad_scale, ema_decay, stream
    assert protos["cdm_adam_ema"] == [vp, vp, vp, vp, vp, ll, vp, vp, i, d, d, d, f, vp, vp]
    # c, B, ncf, p_drop, seed, sub, sub_dev, c_out, keep, stream
    assert protos["cdm_context_drop"] == [vp, i, i, f, ull, ui, vp, vp, vp, vp]
    # cdm_adam_ema is cdm_adam's argument list with ema after v and ema_decay before the stream
    adam = list(protos["cdm_adam"])
    assert protos["cdm_adam_ema"] == adam[:4] + [vp] + adam[4:-1] + [vp] + adam[-1:]


def test_trainer_keyword_arguments_and_methods():
    from cdm_amd import Trainer
    sig = inspect.signature(Trainer.__init__).parameters
    assert sig["ema_decay"].default is None
    assert sig["p_uncond"].default == 0.0
    for name in ("set_ema_decay", "ema_state_dict", "ema_weights", "state_dict", "load_state_dict"):
        assert callable(getattr(Trainer, name)), name
