"""Every byte of the messages behind the learned stack's argument checks (csrc/api.hip): the module entry points, their byte
forms, ReferenceLoss, the four *_create / *_destroy pairs and the MLP's rows checks.  The failing calls need no device:
host buffers stand in for the pointers and small packed structs for the handles, as in tests/test_cabi_gated_u8.py.

EXPECTED was recorded from a build of the commit BEFORE these checks were folded into shared helpers (the library of that
commit, built in a scratch copy, run through cases() below), not from the code under test: the helpers put the messages
together from pieces, and this file pins that the pieces give the text each entry point had."""
import ctypes
import struct

import pytest

import underwater_image_enhancement_amd as uw

LOSS_IDENTITY, LOSS_VGG, LOSS_GATED = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    uw.build()
    return uw.load()


def vp(b):
    return ctypes.cast(b, ctypes.c_void_p) if b is not None else None


def cases(lib):
    """[(id, thunk)]: each thunk makes one failing call and returns its code."""
    ctx, img, out, par, sav, ws, ref = (ctypes.create_string_buffer(1 << 16) for _ in range(7))
    big = 1 << 40
    # stand-ins for the handles: {int device; (padding); the network's leading ints}.  uwie_mlp / uwie_mlp_trainer: F, H, nb
    net, net5 = (ctypes.create_string_buffer(struct.pack("i4xiii", d, 79, 256, 3), 512) for d in (0, 5))
    odd = ctypes.c_void_p(ctypes.addressof(img) + 1)
    odd4 = ctypes.c_void_p(ctypes.addressof(img) + 4)
    out_h = ctypes.c_void_p(1)
    c = []

    def add(name, fn):
        c.append((name, fn))

    # ---- the six float entry points of the two modules
    for name in ("diff_enhance", "diff_gated"):
        bad = 4 if name == "diff_enhance" else 1
        fwd, save, bwd = (getattr(lib, f"uwie_{name}{sfx}_f32") for sfx in ("", "_save", "_bwd"))
        add(f"{name}/null_ctx", lambda f=fwd: f(None, vp(img), vp(out), 1, 8, 8, 0, vp(par), 0, vp(ws), big, None))
        add(f"{name}/null_ptr", lambda f=fwd: f(vp(ctx), vp(img), None, 1, 8, 8, 0, vp(par), 0, vp(ws), big, None))
        add(f"{name}/shape", lambda f=fwd: f(vp(ctx), vp(img), vp(out), 0, 8, 8, 0, vp(par), 0, vp(ws), big, None))
        add(f"{name}/flags", lambda f=fwd, b=bad: f(vp(ctx), vp(img), vp(out), 1, 8, 8, 0, vp(par), b, vp(ws), big, None))
        add(f"{name}/ws", lambda f=fwd: f(vp(ctx), vp(img), vp(out), 1, 8, 8, 0, vp(par), 0, vp(ws), 1, None))
        add(f"{name}_save/null_ctx", lambda f=save: f(None, vp(img), vp(out), 1, 8, 8, 0, vp(par), 0, vp(sav), vp(ws), big, None))
        add(f"{name}_save/null_ptr", lambda f=save: f(vp(ctx), vp(img), vp(out), 1, 8, 8, 0, vp(par), 0, None, vp(ws), big, None))
        add(f"{name}_save/flags", lambda f=save, b=bad: f(vp(ctx), vp(img), vp(out), 1, 8, 8, 0, vp(par), b, vp(sav), vp(ws), big, None))
        add(f"{name}_save/ws", lambda f=save: f(vp(ctx), vp(img), vp(out), 1, 8, 8, 0, vp(par), 0, vp(sav), vp(ws), 1, None))
        add(f"{name}_bwd/null_ctx", lambda f=bwd: f(None, vp(img), vp(par), 0, 0, 1, 8, 8, vp(sav), vp(ref), vp(out), vp(out), vp(ws), big, None))
        add(f"{name}_bwd/null_ptr", lambda f=bwd: f(vp(ctx), vp(img), vp(par), 0, 0, 1, 8, 8, vp(sav), vp(ref), vp(out), None, vp(ws), big, None))
        add(f"{name}_bwd/flags", lambda f=bwd, b=bad: f(vp(ctx), vp(img), vp(par), b, 0, 1, 8, 8, vp(sav), vp(ref), vp(out), vp(par), vp(ws), big, None))
        add(f"{name}_bwd/alias", lambda f=bwd: f(vp(ctx), vp(img), vp(par), 0, 0, 1, 8, 8, vp(sav), vp(ref), vp(img), vp(par), vp(ws), big, None))
        add(f"{name}_bwd/ws", lambda f=bwd: f(vp(ctx), vp(img), vp(par), 0, 0, 1, 8, 8, vp(sav), vp(ref), vp(out), vp(par), vp(ws), 1, None))

    # ---- the two byte entry points
    for name, bad in (("diff_enhance_u8", 4), ("diff_gated_u8", 1)):
        f = getattr(lib, f"uwie_{name}")
        add(f"{name}/null_ctx", lambda f=f: f(None, vp(img), vp(out), None, 1, 8, 8, vp(par), 0, None, vp(ws), big, None))
        add(f"{name}/null_ptr", lambda f=f: f(vp(ctx), vp(img), vp(out), None, 1, 8, 8, None, 0, None, vp(ws), big, None))
        add(f"{name}/no_output", lambda f=f: f(vp(ctx), vp(img), None, None, 1, 8, 8, vp(par), 0, None, vp(ws), big, None))
        add(f"{name}/misaligned", lambda f=f: f(vp(ctx), odd, vp(out), None, 1, 8, 8, vp(par), 0, None, vp(ws), big, None))
        add(f"{name}/shape", lambda f=f: f(vp(ctx), vp(img), vp(out), None, 1, 0, 8, vp(par), 0, None, vp(ws), big, None))
        add(f"{name}/batch_65536", lambda f=f: f(vp(ctx), vp(img), vp(out), None, 65536, 1, 1, vp(par), 0, None, vp(ws), 1, None))
        add(f"{name}/flags", lambda f=f, b=bad: f(vp(ctx), vp(img), vp(out), None, 1, 8, 8, vp(par), b, None, vp(ws), big, None))
        add(f"{name}/ws", lambda f=f: f(vp(ctx), vp(img), vp(out), None, 1, 8, 8, vp(par), 0, None, vp(ws), 16, None))
        add(f"{name}/ws_null", lambda f=f: f(vp(ctx), vp(img), vp(out), None, 1, 8, 8, vp(par), 0, None, None, big, None))

    # ---- ReferenceLoss, which takes either module
    rl, rlb = lib.uwie_ref_loss_f32, lib.uwie_ref_loss_bwd_f32
    add("ref_loss/null_ctx", lambda: rl(None, LOSS_VGG, vp(img), vp(par), 0, 0, 1, 8, 8, vp(ref), vp(out), vp(sav), vp(par), vp(ws), big, None))
    add("ref_loss/map", lambda: rl(vp(ctx), 3, vp(img), vp(par), 0, 0, 1, 8, 8, vp(ref), vp(out), vp(sav), vp(par), vp(ws), big, None))
    add("ref_loss/null_params", lambda: rl(vp(ctx), LOSS_VGG, vp(img), None, 0, 0, 1, 8, 8, vp(ref), vp(out), vp(sav), vp(par), vp(ws), big, None))
    add("ref_loss/vgg_flags", lambda: rl(vp(ctx), LOSS_VGG, vp(img), vp(par), 4, 0, 1, 8, 8, vp(ref), vp(out), vp(sav), vp(par), vp(ws), big, None))
    add("ref_loss/gated_flags", lambda: rl(vp(ctx), LOSS_GATED, vp(img), vp(par), 1, 0, 1, 8, 8, vp(ref), vp(out), vp(sav), vp(par), vp(ws), big, None))
    add("ref_loss/ws", lambda: rl(vp(ctx), LOSS_GATED, vp(img), vp(par), 0, 0, 1, 8, 8, vp(ref), vp(out), vp(sav), vp(par), vp(ws), 1, None))
    add("ref_loss_bwd/vgg_flags", lambda: rlb(vp(ctx), LOSS_VGG, vp(img), vp(par), -1, 0, 1, 8, 8, vp(sav), vp(ref), None, vp(par), vp(out),
                                              vp(par), vp(ws), big, None))
    add("ref_loss_bwd/gated_flags", lambda: rlb(vp(ctx), LOSS_GATED, vp(img), vp(par), 2, 0, 1, 8, 8, vp(sav), vp(ref), None, vp(par), vp(out),
                                                vp(par), vp(ws), big, None))
    add("ref_loss_bwd/ws", lambda: rlb(vp(ctx), LOSS_VGG, vp(img), vp(par), 3, 0, 1, 8, 8, vp(sav), vp(ref), None, vp(par), vp(out), vp(par),
                                       vp(ws), 1, None))

    # ---- the creates, and what reads a handle's device
    add("vgg_create/null_ctx", lambda: lib.uwie_vgg_create(None, vp(par), 0, ctypes.byref(out_h)))
    add("vgg_create/precision", lambda: lib.uwie_vgg_create(vp(ctx), vp(par), 2, ctypes.byref(out_h)))
    add("param_net_create/null_ptr", lambda: lib.uwie_param_net_create(vp(ctx), None, 1, ctypes.byref(out_h)))
    add("mlp_create/null_ptr", lambda: lib.uwie_mlp_create(vp(ctx), vp(par), 79, 256, 3, None))
    add("mlp_create/dims", lambda: lib.uwie_mlp_create(vp(ctx), vp(par), 79, 255, 3, ctypes.byref(out_h)))
    add("mlp_trainer_create/null_ctx", lambda: lib.uwie_mlp_trainer_create(None, vp(par), 79, 256, 3, ctypes.byref(out_h)))
    add("mlp_trainer_create/dims", lambda: lib.uwie_mlp_trainer_create(vp(ctx), vp(par), 79, 256, 65, ctypes.byref(out_h)))
    add("model_create/null_ctx", lambda: lib.uwie_model_create(None, None, ctypes.byref(out_h)))
    add("model_info/null", lambda: lib.uwie_model_info(None, None, None, None))
    add("perceptual/other_device", lambda: lib.uwie_perceptual_f32(vp(ctx), vp(net5), vp(img), vp(ref), 1, 8, 8, vp(par), vp(ws), big, None))
    add("perceptual_bwd/other_device", lambda: lib.uwie_perceptual_bwd_f32(vp(ctx), vp(net5), 1, 8, 8, vp(par), vp(out), vp(ws), big, None))
    add("param_net/other_device", lambda: lib.uwie_param_net_f32(vp(ctx), vp(net5), vp(img), None, 1, 8, 8, vp(out), None, vp(ws), big, None))
    add("classify/other_device", lambda: lib.uwie_classify_f64(vp(ctx), vp(net5), vp(img), 1, 79, vp(out), vp(par), None))
    add("predict/other_device", lambda: lib.uwie_predict_strategy_u8(vp(ctx), vp(net5), vp(img), None, 1, 8, 8, 15, vp(out), vp(par), None,
                                                                     vp(ws), big, None))
    add("mlp_trainer_get/null", lambda: lib.uwie_mlp_trainer_get(None, 0, vp(out)))
    add("mlp_trainer_set/which", lambda: lib.uwie_mlp_trainer_set(vp(net), 4, vp(out)))
    add("mlp_trainer_set_step_count/null", lambda: lib.uwie_mlp_trainer_set_step_count(None, 0))

    # ---- rows of the MLP: the eval limit 2^20 (uwie_mlp_forward, uwie_mlp_trainer_eval), the training limit 65536
    for name in ("mlp_forward", "mlp_trainer_eval"):
        f = getattr(lib, f"uwie_{name}")
        call = lambda c_, n_, r_, b_, o_, wb, f=f: f(vp(c_), vp(n_), r_, 1, b_, vp(o_), vp(ws), wb, None)  # noqa: E731
        add(f"{name}/null_ctx", lambda call=call: call(None, net, vp(img), 4, out, big))
        add(f"{name}/null_handle", lambda call=call: call(ctx, None, vp(img), 4, out, big))
        add(f"{name}/null_out", lambda call=call: call(ctx, net, vp(img), 4, None, big))
        add(f"{name}/other_device", lambda call=call: call(ctx, net5, vp(img), 4, out, big))
        add(f"{name}/batch_0", lambda call=call: call(ctx, net, vp(img), 0, out, big))
        add(f"{name}/batch_over", lambda call=call: call(ctx, net, vp(img), (1 << 20) + 1, out, big))
        add(f"{name}/misaligned", lambda call=call: call(ctx, net, odd4, 4, out, big))
        add(f"{name}/ws", lambda call=call: call(ctx, net, vp(img), 4, out, 16))
    tf, tb = lib.uwie_mlp_train_forward, lib.uwie_mlp_backward
    fwd = lambda c_, n_, r_, b_, o_, wb, p=0.3, mode=1: tf(vp(c_), vp(n_), r_, 1, b_, p, mode, None, 0, vp(o_), vp(ws), wb, None)  # noqa: E731
    bwd = lambda c_, n_, r_, b_, g_, wb: tb(vp(c_), vp(n_), r_, 1, b_, vp(g_), vp(ws), wb, None)  # noqa: E731
    for name, call in (("mlp_train_forward", fwd), ("mlp_backward", bwd)):
        add(f"{name}/null_ctx", lambda call=call: call(None, net, vp(img), 4, out, big))
        add(f"{name}/null_rows", lambda call=call: call(ctx, net, None, 4, out, big))
        add(f"{name}/other_device", lambda call=call: call(ctx, net5, vp(img), 4, out, big))
        add(f"{name}/batch_0", lambda call=call: call(ctx, net, vp(img), 0, out, big))
        add(f"{name}/batch_over", lambda call=call: call(ctx, net, vp(img), 65537, out, big))
        add(f"{name}/misaligned", lambda call=call: call(ctx, net, odd4, 4, out, big))
    add("mlp_train_forward/misaligned_out", lambda: fwd(ctx, net, vp(img), 4, ctypes.c_void_p(ctypes.addressof(out) + 2), big))
    add("mlp_train_forward/p", lambda: fwd(ctx, net, vp(img), 4, out, big, p=1.0))
    add("mlp_train_forward/mask_mode", lambda: fwd(ctx, net, vp(img), 4, out, big, mode=2))
    add("mlp_train_forward/ws", lambda: fwd(ctx, net, vp(img), 4, out, 16))
    add("mlp_backward/no_forward", lambda: bwd(ctx, net, vp(img), 4, out, big))
    return c


EXPECTED = {
    'diff_enhance/null_ctx': (-1, 'diff_enhance: NULL pointer'),
    'diff_enhance/null_ptr': (-1, 'diff_enhance: NULL pointer'),
    'diff_enhance/shape': (-1, 'batch/H/W out of range'),
    'diff_enhance/flags': (-1, 'diff_enhance: flags are UWIE_DIFF_OMEGA | UWIE_DIFF_GAMMA'),
    'diff_enhance/ws': (-2, 'workspace too small: need 12781568 bytes, got 1'),
    'diff_enhance_save/null_ctx': (-1, 'diff_enhance_save: NULL pointer'),
    'diff_enhance_save/null_ptr': (-1, 'diff_enhance_save: NULL pointer'),
    'diff_enhance_save/flags': (-1, 'diff_enhance_save: flags are UWIE_DIFF_OMEGA | UWIE_DIFF_GAMMA'),
    'diff_enhance_save/ws': (-2, 'workspace too small: need 12781568 bytes, got 1'),
    'diff_enhance_bwd/null_ctx': (-1, 'diff_enhance_bwd: NULL pointer'),
    'diff_enhance_bwd/null_ptr': (-1, 'diff_enhance_bwd: NULL pointer'),
    'diff_enhance_bwd/flags': (-1, 'diff_enhance_bwd: flags are UWIE_DIFF_OMEGA | UWIE_DIFF_GAMMA'),
    'diff_enhance_bwd/alias': (-1, 'diff_enhance_bwd: d_grad_img must not alias d_img or d_grad_out'),
    'diff_enhance_bwd/ws': (-2, 'workspace too small: need 512 bytes, got 1'),
    'diff_gated/null_ctx': (-1, 'diff_gated: NULL pointer'),
    'diff_gated/null_ptr': (-1, 'diff_gated: NULL pointer'),
    'diff_gated/shape': (-1, 'batch/H/W out of range'),
    'diff_gated/flags': (-1, 'diff_gated: flags are reserved (0)'),
    'diff_gated/ws': (-2, 'workspace too small: need 12781568 bytes, got 1'),
    'diff_gated_save/null_ctx': (-1, 'diff_gated_save: NULL pointer'),
    'diff_gated_save/null_ptr': (-1, 'diff_gated_save: NULL pointer'),
    'diff_gated_save/flags': (-1, 'diff_gated_save: flags are reserved (0)'),
    'diff_gated_save/ws': (-2, 'workspace too small: need 12781568 bytes, got 1'),
    'diff_gated_bwd/null_ctx': (-1, 'diff_gated_bwd: NULL pointer'),
    'diff_gated_bwd/null_ptr': (-1, 'diff_gated_bwd: NULL pointer'),
    'diff_gated_bwd/flags': (-1, 'diff_gated_bwd: flags are reserved (0)'),
    'diff_gated_bwd/alias': (-1, 'diff_gated_bwd: d_grad_img must not alias d_img or d_grad_out'),
    'diff_gated_bwd/ws': (-2, 'workspace too small: need 512 bytes, got 1'),
    'diff_enhance_u8/null_ctx': (-1, 'diff_enhance_u8: NULL pointer'),
    'diff_enhance_u8/null_ptr': (-1, 'diff_enhance_u8: NULL pointer'),
    'diff_enhance_u8/no_output': (-1, 'diff_enhance_u8: at least one of d_out_u8, d_out_f32'),
    'diff_enhance_u8/misaligned': (-1, 'diff_enhance_u8: d_in must be 4-byte aligned'),
    'diff_enhance_u8/shape': (-1, 'batch/H/W out of range'),
    'diff_enhance_u8/batch_65536': (-2, 'workspace too small: need 202899456 bytes, got 1'),
    'diff_enhance_u8/flags': (-1, 'diff_enhance_u8: flags are UWIE_DIFF_OMEGA | UWIE_DIFF_GAMMA'),
    'diff_enhance_u8/ws': (-2, 'workspace too small: need 3328 bytes, got 16'),
    'diff_enhance_u8/ws_null': (-2, 'workspace too small: need 3328 bytes, got 1099511627776'),
    'diff_gated_u8/null_ctx': (-1, 'diff_gated_u8: NULL pointer'),
    'diff_gated_u8/null_ptr': (-1, 'diff_gated_u8: NULL pointer'),
    'diff_gated_u8/no_output': (-1, 'diff_gated_u8: at least one of d_out_u8, d_out_f32'),
    'diff_gated_u8/misaligned': (-1, 'diff_gated_u8: d_in must be 4-byte aligned'),
    'diff_gated_u8/shape': (-1, 'batch/H/W out of range'),
    'diff_gated_u8/batch_65536': (-1, 'diff_gated_u8: batch is at most 65535'),
    'diff_gated_u8/flags': (-1, 'diff_gated_u8: flags are reserved (0)'),
    'diff_gated_u8/ws': (-2, 'workspace too small: need 6912 bytes, got 16'),
    'diff_gated_u8/ws_null': (-2, 'workspace too small: need 6912 bytes, got 1099511627776'),
    'ref_loss/null_ctx': (-1, 'ref_loss: NULL pointer'),
    'ref_loss/map': (-1, 'ref_loss: map is UWIE_LOSS_IDENTITY, UWIE_LOSS_VGG or UWIE_LOSS_GATED'),
    'ref_loss/null_params': (-1, 'ref_loss: NULL pointer (d_params, d_saved)'),
    'ref_loss/vgg_flags': (-1, 'ref_loss: vgg flags are UWIE_DIFF_OMEGA | UWIE_DIFF_GAMMA'),
    'ref_loss/gated_flags': (-1, 'ref_loss: gated flags are reserved (0)'),
    'ref_loss/ws': (-2, 'workspace too small: need 12781824 bytes, got 1'),
    'ref_loss_bwd/vgg_flags': (-1, 'ref_loss: vgg flags are UWIE_DIFF_OMEGA | UWIE_DIFF_GAMMA'),
    'ref_loss_bwd/gated_flags': (-1, 'ref_loss: gated flags are reserved (0)'),
    'ref_loss_bwd/ws': (-2, 'workspace too small: need 512 bytes, got 1'),
    'vgg_create/null_ctx': (-1, 'vgg_create: NULL pointer'),
    'vgg_create/precision': (-1, 'vgg_create: precision is UWIE_VGG_F32 or UWIE_VGG_F16'),
    'param_net_create/null_ptr': (-1, 'param_net_create: NULL pointer'),
    'mlp_create/null_ptr': (-1, 'mlp_create: NULL pointer'),
    'mlp_create/dims': (-1, 'mlp_create: feature_dim 1 .. 1152, hidden_dim even 2 .. 1152, num_blocks 0 .. 64'),
    'mlp_trainer_create/null_ctx': (-1, 'mlp_trainer_create: NULL pointer'),
    'mlp_trainer_create/dims': (-1, 'mlp_trainer_create: feature_dim 1 .. 1152, hidden_dim even 2 .. 1152, num_blocks 0 .. 64'),
    'model_create/null_ctx': (-1, 'model_create: NULL context or out_model'),
    'model_info/null': (-1, 'model_info: NULL model'),
    'perceptual/other_device': (-1, 'perceptual: the network lives on another device'),
    'perceptual_bwd/other_device': (-1, 'perceptual: the network lives on another device'),
    'param_net/other_device': (-1, 'param_net: the network lives on another device'),
    'classify/other_device': (-1, 'classify: the model lives on another device'),
    'predict/other_device': (-1, 'predict: the model lives on another device'),
    'mlp_trainer_get/null': (-1, 'mlp_trainer_get: NULL or misaligned pointer, or which outside UWIE_TRAINER_PARAMS .. UWIE_TRAINER_EXP_AVG_SQ'),
    'mlp_trainer_set/which': (-1, 'mlp_trainer_set: NULL or misaligned pointer, or which outside UWIE_TRAINER_PARAMS .. UWIE_TRAINER_EXP_AVG_SQ'),
    'mlp_trainer_set_step_count/null': (-1, 'mlp_trainer_set_step_count: NULL trainer'),
    'mlp_forward/null_ctx': (-1, 'mlp_forward: NULL pointer'),
    'mlp_forward/null_handle': (-1, 'mlp_forward: NULL pointer'),
    'mlp_forward/null_out': (-1, 'mlp_forward: NULL pointer'),
    'mlp_forward/other_device': (-1, 'mlp_forward: the network lives on another device'),
    'mlp_forward/batch_0': (-1, 'mlp_forward: batch out of range (1 .. 2^20)'),
    'mlp_forward/batch_over': (-1, 'mlp_forward: batch out of range (1 .. 2^20)'),
    'mlp_forward/misaligned': (-1, 'mlp_forward: d_features and d_out must be aligned for their element types'),
    'mlp_forward/ws': (-2, 'workspace too small: need 14336 bytes, got 16'),
    'mlp_trainer_eval/null_ctx': (-1, 'mlp_trainer_eval: NULL pointer'),
    'mlp_trainer_eval/null_handle': (-1, 'mlp_trainer_eval: NULL pointer'),
    'mlp_trainer_eval/null_out': (-1, 'mlp_trainer_eval: NULL pointer'),
    'mlp_trainer_eval/other_device': (-1, 'mlp_trainer_eval: the trainer lives on another device'),
    'mlp_trainer_eval/batch_0': (-1, 'mlp_trainer_eval: batch out of range (1 .. 2^20)'),
    'mlp_trainer_eval/batch_over': (-1, 'mlp_trainer_eval: batch out of range (1 .. 2^20)'),
    'mlp_trainer_eval/misaligned': (-1, 'mlp_trainer_eval: d_features and d_out must be aligned for their element types'),
    'mlp_trainer_eval/ws': (-2, 'workspace too small: need 14336 bytes, got 16'),
    'mlp_train_forward/null_ctx': (-1, 'mlp_train_forward: NULL pointer'),
    'mlp_train_forward/null_rows': (-1, 'mlp_train_forward: NULL pointer'),
    'mlp_train_forward/other_device': (-1, 'mlp_train_forward: the trainer lives on another device'),
    'mlp_train_forward/batch_0': (-1, 'mlp_train_forward: batch out of range (1 .. 65536)'),
    'mlp_train_forward/batch_over': (-1, 'mlp_train_forward: batch out of range (1 .. 65536)'),
    'mlp_train_forward/misaligned': (-1, 'mlp_train_forward: d_features and d_out must be aligned for their element types'),
    'mlp_backward/null_ctx': (-1, 'mlp_backward: NULL pointer'),
    'mlp_backward/null_rows': (-1, 'mlp_backward: NULL pointer'),
    'mlp_backward/other_device': (-1, 'mlp_backward: the trainer lives on another device'),
    'mlp_backward/batch_0': (-1, 'mlp_backward: batch out of range (1 .. 65536)'),
    'mlp_backward/batch_over': (-1, 'mlp_backward: batch out of range (1 .. 65536)'),
    'mlp_backward/misaligned': (-1, 'mlp_backward: d_features and d_grad_out must be aligned for their element types'),
    'mlp_train_forward/misaligned_out': (-1, 'mlp_train_forward: d_features and d_out must be aligned for their element types'),
    'mlp_train_forward/p': (-1, 'mlp_train_forward: the dropout rate p must lie in [0, 1)'),
    'mlp_train_forward/mask_mode': (-1, 'mlp_train_forward: mask_mode is UWIE_MASKS_GIVEN or UWIE_MASKS_DRAWN'),
    'mlp_train_forward/ws': (-2, 'workspace too small: need 45312 bytes, got 16'),
    'mlp_backward/no_forward': (-1, 'mlp_backward: no uwie_mlp_train_forward of this batch precedes it'),
}


def test_every_case_has_its_literal(lib):
    assert [name for name, _ in cases(lib)] == list(EXPECTED)


@pytest.mark.parametrize("name", list(EXPECTED))
def test_message(lib, name):
    code = dict(cases(lib))[name]()
    assert (code, lib.uwie_last_error().decode()) == EXPECTED[name]
