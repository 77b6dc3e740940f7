"""CPU: host-side logic of the product package -- library loads and exports every declared symbol, reference-compatible
constructor / state_dict layout / init, config quirks (time_steps rounding), error behaviour, and the no-CPU-fallback rule."""
import json
import os

import pytest
import torch

from mridc_amd import _lib
from tests._util import T, meta, weights

CIRIM_CFG = dict(recurrent_layer="IndRNN", conv_filters=[64, 64, 2], conv_kernels=[5, 3, 3], conv_dilations=[1, 2, 1],
                 conv_bias=[True, True, False], recurrent_filters=[64, 64, 0], recurrent_kernels=[1, 1, 0],
                 recurrent_dilations=[1, 1, 0], recurrent_bias=[True, True, False], depth=2, time_steps=5, conv_dim=2,
                 num_cascades=8, no_dc=True, keep_eta=True, fft_centered=False, fft_normalization="backward",
                 spatial_dims=[-2, -1], coil_dim=1, dimensionality=2, coil_combination_method="SENSE",
                 train_loss_fn="l1", val_loss_fn="l1")


def test_library_loads_and_exports_every_declared_symbol():
    assert os.path.exists(_lib.LIB_PATH), "build first: python -m mridc_amd._build"
    L = _lib.lib()
    declared = _lib.declared_symbols()
    assert len(declared) >= 30
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/mridc_amd.h but not exported"
    assert set(declared) == set(_lib._SIGNATURES), "ctypes signature table out of sync with the header"
    assert L.mrx_version() >= 100
    assert L.mrx_fft_max_len() >= 640


def test_no_cpu_fallback():
    import mridc_amd.collections.common.parts.fft as fft
    import mridc_amd.collections.common.parts.utils as utils
    x = torch.zeros(2, 4, 4, 2)
    for fn in (lambda: fft.fft2(x), lambda: fft.ifft2(x), lambda: fft.fftshift(x), lambda: utils.complex_mul(x, x),
               lambda: utils.complex_abs(x), lambda: utils.rss(x, 0), lambda: utils.sense(x, x, 0)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn()


def test_product_never_imports_oracle():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for dp, _, files in os.walk(os.path.join(root, "mridc_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dp, f)).read()
                assert "import oracle" not in src and "from oracle" not in src, f"{f} imports the oracle"


def test_error_behaviour_matches_reference():
    import mridc_amd.collections.common.parts.fft as fft
    import mridc_amd.collections.common.parts.utils as utils
    x3 = torch.zeros(2, 4, 4, 3)
    x = torch.zeros(2, 4, 4, 2)
    with pytest.raises(ValueError, match="separate complex dim"):
        utils.complex_mul(x3, x3)
    with pytest.raises(ValueError, match="separate complex dim"):
        utils.complex_conj(x3)
    with pytest.raises(ValueError, match="separate complex dim"):
        utils.complex_abs(x3)
    with pytest.raises(ValueError, match="separate complex dim"):
        utils.complex_abs_sq(x3)
    with pytest.raises(ValueError, match="Output type not supported."):
        utils.coil_combination(x, x, "FOO", 0)
    with pytest.raises(ValueError, match="len\\(shift\\) must match len\\(dim\\)"):
        fft.roll(x, [1, 2], [0])
    with pytest.raises(ValueError, match="Invalid shapes."):
        utils.center_crop(x[..., 0], (5, 1))
    with pytest.raises(ValueError, match="Invalid shapes."):
        utils.complex_center_crop(x, (1, 9))
    from mridc_amd.collections.reconstruction.models.rim.rim_block import RIMBlock
    cfg = {k: CIRIM_CFG[k] for k in ("conv_filters", "conv_kernels", "conv_dilations", "conv_bias", "recurrent_filters",
                                     "recurrent_kernels", "recurrent_dilations", "recurrent_bias")}
    with pytest.raises(ValueError, match="Please specify a proper recurrent layer type."):
        RIMBlock(recurrent_layer="LSTM", **cfg)
    from mridc_amd.collections.reconstruction.models.unet_base.unet_block import NormUnet
    with pytest.raises(AssertionError):
        NormUnet.complex_to_chan_dim(torch.zeros(1, 1, 4, 4, 3))
    assert utils.is_none(None) and utils.is_none("None") and not utils.is_none(0)


def test_crops_are_views_with_reference_offsets(golden):
    import mridc_amd.collections.common.parts.utils as utils
    z = golden("g3_complex.npz")
    img = T(z["crop/x"])
    assert torch.equal(utils.center_crop(img, (7, 8)), T(z["crop/center_7_8"]))
    assert torch.equal(utils.center_crop(img, (10, 13)), T(z["crop/center_10_13"]))
    assert torch.equal(utils.complex_center_crop(T(z["crop/cx"]), (6, 9)), T(z["crop/complex_6_9"]))


def test_cirim_config_quirks_and_state_dict_layout():
    from mridc_amd.collections.reconstruction.models.cirim import CIRIM
    m = CIRIM(CIRIM_CFG)
    assert m.time_steps == 8                               # 5 -> 8 (cirim.py:50-51)
    assert all(b.time_steps == 8 for b in m.cirim)
    assert CIRIM(dict(CIRIM_CFG, time_steps=9, num_cascades=1)).time_steps == 16
    assert sum(p.numel() for p in m.parameters()) == 423_937
    keys = set(m.state_dict().keys())
    assert "dc_weight" in keys and "cirim.7.final_layer.0.conv_layer.weight" in keys
    assert tuple(m.state_dict()["cirim.0.layers.0.rnn.hh"].shape) == (1, 64, 1, 1)
    assert tuple(m.state_dict()["cirim.0.layers.1.convs.conv_layer.weight"].shape) == (64, 64, 3, 3)
    import types
    assert isinstance(m.forward(None, None, None, None, None), types.GeneratorType)     # cirim.py:165 yields


def test_rimblock_init_is_bit_identical_to_reference(golden):
    """Same module hierarchy + same init calls in the same order => same weights under the same seed as the reference
    (golden g5 'ind64' was created with torch.manual_seed(500), 'gru16' with 504, 'mgu16' with 506; IndRNN cases then
    had ih/hh scaled, so compare the unscaled parameters only)."""
    from mridc_amd.collections.reconstruction.models.rim.rim_block import RIMBlock
    z = golden("g5_rimblock.npz")
    for nm, seed in (("ind64", 500), ("gru16", 504), ("mgu16", 506)):
        cfg = meta(z, f"{nm}/cfg")
        torch.manual_seed(seed)
        blk = RIMBlock(**cfg)
        ref = weights(z, f"{nm}/w/")
        sd = blk.state_dict()
        assert set(sd.keys()) == set(ref.keys()), nm
        for k, v in ref.items():
            assert torch.equal(sd[k], v), f"{nm}: {k} differs from the reference initialisation"
        blk.load_state_dict(ref)                            # reference checkpoints drop in


def test_varnet_state_dict_loads_reference_weights(golden):
    from mridc_amd.collections.reconstruction.models.vn import VarNet
    from mridc_amd.collections.reconstruction.models.unet import UNet
    z = golden("g8_models.npz")
    cfg = meta(z, "vn/cfg")
    m = VarNet(cfg)
    sd = weights(z, "vn/w/")
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert unexpected == [] and missing == ["dc_weight"]      # model-level dc_weight (vn.py:91) is not in the block dumps
    u = UNet(meta(z, "unet/cfg"))
    u.load_state_dict(weights(z, "unet/w/"))


def test_default_paths_are_the_fused_ones():
    """Host-side routing (no compute): the headline CIRIM config takes the split-bf16 layer with the final convolution in its tail and in-place
    states, the reference U-Net shapes take the kernels that normalise on load -- so the `-m gpu` parity tests exercise what ships -- and a
    configuration outside those shapes falls back (rim_block.py:121, unet_block.py:139-227)."""
    from mridc_amd import ops, synthetic
    from mridc_amd.collections.reconstruction.models.cirim import CIRIM
    from mridc_amd.collections.reconstruction.models.rim.rim_block import RIMBlock
    from mridc_amd.collections.reconstruction.models.unet_base.unet_block import NormUnet, Unet
    blk = CIRIM(dict(synthetic.CIRIM_BASELINE_CFG, num_cascades=1)).cirim[0]
    assert RIMBlock.layer2_sb and RIMBlock.fused_final and RIMBlock.inplace_state
    assert blk._sb_layer(blk.layers[1]) and not blk._sb_layer(blk.layers[0]) and blk._tail_fused()
    gru = CIRIM(dict(synthetic.CIRIM_BASELINE_CFG, num_cascades=1, recurrent_layer="GRU")).cirim[0]
    assert not gru._tail_fused()                                   # gated cells keep the stand-alone final convolution
    assert ops.conv3x3_sb_supported(64, 64, 3, 1) and ops.conv3x3_sb_supported(64, 64, 3, 2)
    assert not ops.conv3x3_sb_supported(64, 128, 3, 1) and not ops.conv3x3_sb_supported(64, 64, 5, 1)
    assert ops.conv3x3_taps_supported(128, 4) and ops.conv3x3_taps_supported(64, 2) and not ops.conv3x3_taps_supported(64, 8)
    assert not ops.conv3x3_taps_supported(56, 2)
    for chans, pools in ((14, 2), (18, 4), (32, 4)):
        net = NormUnet(chans, pools).eval()
        assert Unet.fused and net.unet._fusable()
        with torch.no_grad():                                      # (with gradients recorded the differentiable forms run instead)
            assert net._fused_ok(torch.zeros(1, 1, 8, 8, 2)) and not net._fused_ok(torch.zeros(1, 2, 8, 8))
        assert not net._fused_ok(torch.zeros(1, 1, 8, 8, 2))
    wide = Unet(2, 8, chans=8, num_pool_layers=2).eval()           # 8 output channels: the closing 1x1 kernel covers <= 4
    assert not wide._fusable()
    assert ops.rim_layer1_inplace_ok(4, 64, 5, 1) and not ops.rim_layer1_inplace_ok(4, 64, 3, 1)


def test_bench_and_tests_state_the_same_training_tolerances():
    import importlib.util
    import os
    from tests._util import TRAIN_TOL
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert bench.TRAIN_TOL == TRAIN_TOL


def test_bench_default_batch_per_configuration(monkeypatch):
    """The step of the driver's command: slices per launch and streams the bench picks when no flag says otherwise (a slice is 480
    tiles of the persistent layer kernels -- 8 slices are 15 exact rounds on 256 CUs; the 2-D-mask line stays at 4, where its coil stack still fits the
    Infinity Cache; training is one slice per rank and step, as the reference's trainer feeds it)."""
    import importlib.util
    import os
    import sys
    spec = importlib.util.spec_from_file_location("bench_module_defaults", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)

    def defaults(*flags):
        monkeypatch.setattr(sys, "argv", ["bench.py", *flags])
        a = bench.parse()
        return a.batch, a.streams

    assert defaults() == (8, 2)
    assert defaults("--mask", "2d") == (4, 2)
    assert defaults("--model", "e2evn") == (8, 2)
    assert defaults("--model", "qcirim") == (1, 6)            # (six streams: 740 -> 790 slices/s, tools/runs/r06x.sh)
    assert defaults("--train", "--dtype", "bf16") == (1, 2)
    assert defaults("--train", "--model", "e2evn") == (1, 2)
    assert defaults("--rnn", "GRU", "--cascades", "1") == (1, 2)
    assert defaults("--batch", "3", "--streams", "1") == (3, 1)


def test_no_object_of_the_library_contains_packed_fp32_instructions(tmp_path):
    """DESIGN.md 5, "Concurrent streams": no kernel of the library may issue packed-fp32 vector instructions -- on MI355X v_pk_*_f32 with operand
    modifiers returns wrong results while a foreign wave on the same SIMD issues v_mfma_f32_16x16x32_f16 (tools/probe/pk_mfma_repro.hip reproduces it
    without the library).  Guards the build flags: disassembles the device code of EVERY built object and counts v_pk_{add,mul,fma}_f32."""
    import os
    import shutil
    import subprocess
    from mridc_amd import _build
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if not os.path.exists(objdump):
        pytest.skip("no llvm-objdump in this image")
    _build.build()
    names = [os.path.splitext(n)[0] for n, _ in _build.SOURCES if n.endswith(".hip") and os.path.exists(os.path.join(_build.CSRC, n))]
    assert len(names) >= 18 and "fft" in names and "rim_layer2_sb" in names and "unet_fused" in names
    for name in names:
        src = os.path.join(_build.LIBDIR, name + ".o")
        assert os.path.exists(src), src
        obj = shutil.copy(src, str(tmp_path / (name + ".o")))
        subprocess.run([objdump, "--offloading", obj], check=True, capture_output=True, cwd=str(tmp_path))
        dev = [f for f in os.listdir(tmp_path) if f.startswith(name + ".o.") and "amdgcn" in f]
        assert dev, os.listdir(tmp_path)
        asm = subprocess.run([objdump, "-d", str(tmp_path / dev[0])], check=True, capture_output=True, text=True).stdout
        assert "v_mul_f32" in asm or "v_fma_f32" in asm or "v_fmac_f32" in asm          # (the disassembly is that of the kernels)
        packed = [ln for ln in asm.splitlines() if "v_pk_fma_f32" in ln or "v_pk_mul_f32" in ln or "v_pk_add_f32" in ln]
        assert not packed, f"{name}.o: {len(packed)} packed-fp32 instructions, e.g. {packed[0].strip()}"


def test_hot_kernels_keep_their_loads_ahead_of_their_waits(tmp_path):
    """DESIGN.md 7.1 (round 4): on gfx950 `vmcnt` retires in order, and a load whose only use sits behind a branch is waited for in that block -- a loop
    that reads like "thirty loads, then thirty LDS writes" ran as thirty memory round trips (k_pfa372_reduce, k_cols_dc_t4, the gather inside k_llg372,
    k_conv1x1_sb128 ...), and a run-time test inside an unrolled loop left part of layer 1's patch in scratch memory.  Guards what those fixes bought:
    per hot kernel of the built library, the number of load groups that end in `s_waitcnt vmcnt(0)` (tools/probe/load_wait_scan.py's count, here on the
    objects' disassembly) and the scratch size of its kernel descriptor."""
    import os
    import re
    import shutil
    import subprocess
    from mridc_amd import _build
    objdump, readelf = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("no llvm-objdump / llvm-readelf in this image")
    _build.build()
    # object -> [(mangled-name prefix, max groups of <= 2 loads, max groups, scratch must be 0)]   (lib 256: the measured counts + a little room)
    hot = {
        "rim_layer1_sb": [("_Z15k_rim_layer1_sbILb1ELb1ELb0ELi1ELi16EE", 4, 8, True)],                   # 3 / 6
        "rim_layer2_sb": [("_Z15k_rim_layer2_sbILi2ELb1ELb0ELb1ELi0ELb1ELb0ELb0ELb1EE", 6, 11, True)],   # the FAST route (round 5)
        "llg372": [("_Z8k_llg372ILi0ELb1ELb0EE", 0, 2, True), ("_Z8k_llg372ILi0ELb1ELb1EE", 0, 2, True),   # 0 / 1 each (151 loads in the gather form)
                   ("_Z15k_pfa372_reduce", 0, 2, True), ("_Z15k_pfa372_expandILb0ELb0ELb0EE", 0, 2, True),
                   ("_Z15k_pfa372_expandILb0ELb0ELb1EE", 0, 2, True)],      # (<.., GAT>: round 5, the tap gather inside the general-mask gradient's first pass)
        "fft": [("_Z12k_cols_dc_t4I6PlanCTILi640EJLi5ELi8ELi4ELi4EEELb1EE", 0, 2, True)],
        "gated_cell_sb": [("_Z15k_conv1x1_sb128ILi2ELb0EE", 5, 9, True), ("_Z15k_conv1x1_sb128ILi2ELb1EE", 5, 9, True)],   # 4 / 7 (<.., true>: the precision-16 form, round 6)
        "train_bf16": [("_Z13k_tl_cell_bwdILb1ELb1ELb1EE", 3, 6, True)],                                 # 2 / 4
        # (the ticket form of round 5 is its own instantiation, <.., true, ..>; round 6: <.., rows per work item, fp16 terms> -- E2EVN's 14 -> 14 layers run the
        # 16-row form at the bench's batch, the one-term forms are the precision-16 route)
        "unet_f16": [("_Z9k_uconv_hILi4ELi2ELb0ELb0ELi8ELi2EE", 1, 5, True), ("_Z9k_uconv_hILi1ELi1ELb1ELb0ELi8ELi2EE", 1, 4, True),
                     ("_Z9k_uconv_hILi1ELi1ELb1ELb0ELi16ELi2EE", 1, 4, True), ("_Z9k_uconv_hILi1ELi1ELb1ELb0ELi16ELi1EE", 1, 4, True),
                     ("_Z9k_uconv_hILi2ELi1ELb1ELb0ELi8ELi1EE", 1, 4, True)],
    }
    for name, kernels in hot.items():
        obj = shutil.copy(os.path.join(_build.LIBDIR, name + ".o"), str(tmp_path / (name + ".o")))
        subprocess.run([objdump, "--offloading", obj], check=True, capture_output=True, cwd=str(tmp_path))
        dev = [f for f in os.listdir(tmp_path) if f.startswith(name + ".o.") and "amdgcn" in f]
        assert dev, os.listdir(tmp_path)
        asm = subprocess.run([objdump, "-d", str(tmp_path / dev[0])], check=True, capture_output=True, text=True).stdout
        notes = subprocess.run([readelf, "--notes", str(tmp_path / dev[0])], check=True, capture_output=True, text=True).stdout
        scratch = {}
        for blk in notes.split("  - ."):
            n_, p_ = re.search(r"\.name:\s+(\S+)", blk), re.search(r"private_segment_fixed_size:\s+(\d+)", blk)
            if n_ and p_:
                scratch[n_.group(1)] = int(p_.group(1))
        counts, cur, pending = {}, None, 0
        for ln in asm.splitlines():
            m = re.match(r"^[0-9a-f]+ <(_Z\w+)>:", ln)
            if m:
                cur, pending = m.group(1), 0
                counts[cur] = [0, 0]
            elif cur is not None:
                if re.search(r"\b(global_load|buffer_load)", ln):
                    pending += 1
                elif "s_waitcnt" in ln and "vmcnt(0)" in ln:
                    if pending:
                        counts[cur][1] += 1
                        counts[cur][0] += pending <= 2
                    pending = 0
        for prefix, max_short, max_groups, no_scratch in kernels:
            found = [k for k in counts if k.startswith(prefix)]
            assert len(found) == 1, f"{name}.o: {prefix}* matches {found}"
            short, groups = counts[found[0]]
            assert short <= max_short and groups <= max_groups, (
                f"{found[0]}: {groups} load groups end in vmcnt(0), {short} of them of one or two loads (allowed {max_groups} / {max_short}): "
                "some loads are waited for one by one again (python tools/probe/load_wait_scan.py)")
            if no_scratch:
                assert scratch.get(found[0], -1) == 0, f"{found[0]}: {scratch.get(found[0])} bytes of scratch per lane"


# ---- round 5: who owns cached host state -----------------------------------------------------------------------------------
def test_written_pointer_args_cover_every_declared_function():
    """The binding drops operand bounds for every range a call may write: the positions come from the header's const-ness, so each declared
    function must parse, positions must be pointer slots of the ctypes table, and the known producers / consumers must come out right."""
    w = _lib.written_pointer_args()
    assert set(w) == set(_lib._SIGNATURES)
    for name, pos in w.items():
        args = _lib._SIGNATURES[name][0]
        assert all(i < len(args) and args[i] is _lib._p for i in pos), name
    assert w["mrx_conv3x3_sb_chain"] == (4, 6) and w["mrx_conv3x3_h"] == (4,) and w["mrx_fft2"] == (1,) and w["mrx_version"] == ()
    assert w["mrx_rim_layer2_f16_cb8"] == (6, 7)          # h_new and taps, not xmax (read)
    L = _lib.lib()
    assert L.mrx_checks_enabled() in (0, 1)
    assert hasattr(L.mrx_fft2, "raw") and not hasattr(L.mrx_version, "raw")


def test_bound_table_is_keyed_on_memory_not_on_objects():
    """_lib.bound_attach / bound_of / bound_note_write on CPU tensors (the table only looks at addresses, versions and object identity)."""
    _lib._BOUNDS.clear()
    t = torch.zeros(4, 64)
    b = torch.ones(1)
    _lib.bound_attach(t, b)
    assert _lib.bound_of(t) is b
    assert _lib.bound_of(t[:]) is None and _lib.bound_of(t.view(256)) is None          # another object, even over the same bytes: not found
    _lib.bound_note_write(t.data_ptr() + 4096, t.data_ptr() + 8192)                     # a write next to it
    assert _lib.bound_of(t) is b
    p = _lib.ptr(t[2:])                                                                  # the range a call writing a VIEW would report
    assert (p.lo, p.hi) == (t.data_ptr() + 512, t.data_ptr() + 1024)
    _lib.bound_note_write(p.lo, p.hi)
    assert _lib.bound_of(t) is None
    _lib.bound_attach(t, b)
    t.add_(1.0)                                                                          # a torch write: the version moves
    assert _lib.bound_of(t) is None
    _lib.bound_attach(t, b)
    big = torch.zeros(8, 64)
    _lib.bound_attach(big[1:5], b)                                                        # (a temporary view: dead at once)
    assert len(_lib._BOUNDS) == 2 and _lib.bound_of(big[1:5]) is None
    nc = torch.zeros(6, 10)[:, :4]                                                        # non-contiguous: the extent of its strides
    assert _lib._span(nc) == (nc.data_ptr(), nc.data_ptr() + (5 * 10 + 4) * 4)
    for i in range(100):
        _lib.bound_attach(torch.zeros(3), b)
    assert len(_lib._BOUNDS) <= 64
    _lib._BOUNDS.clear()


def test_prelu_slope_cache_dies_with_its_module():
    """The failing sequence behind round 4's one-off 4e-2 error of test_dunet_vs_golden: didn.py kept PReLU slopes in a process-wide dict keyed
    by id(module) and validated by (weight address, weight version).  A model is dropped, the next model's PReLU gets the freed id, its weight
    the freed 512-byte block, the version is equal -- and the dead model's slope is served.  Here the collision is forced (same id by
    construction of the key, same storage through an alias): the cache must live on the module."""
    import gc
    from mridc_amd.collections.reconstruction.models.didn import didn
    a = torch.nn.PReLU(init=0.1)
    assert didn._prelu_slope(a) == pytest.approx(0.1)
    assert not hasattr(didn, "_SLOPES"), "a process-wide slope table keyed by id(module)"
    store = a.weight.detach()                                  # the 'recycled block'
    del a
    gc.collect()
    store.fill_(0.7)
    b = torch.nn.PReLU(init=0.25)
    b.weight.data = store                                      # same address, and b.weight._version == 0 as a's was
    assert didn._prelu_slope(b) == pytest.approx(0.7)
    with torch.no_grad():
        b.weight.fill_(0.3)                                    # an in-place update moves the version
    assert didn._prelu_slope(b) == pytest.approx(0.3)
    b.weight.data = torch.tensor([0.9])                        # a re-pointed parameter moves the address; the old storage stays pinned
    assert didn._prelu_slope(b) == pytest.approx(0.9)


def test_bench_summary_is_the_last_key_and_fits_a_kilobyte():
    """The driver keeps the tail of the bench line: `summary` (bench.summary_of) carries every configuration's value, roofline fraction, counter traffic over
    algorithmic bytes, parity and CPU baseline in <= 1 KB, and bench.main() appends it as the LAST key."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_module2", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    sub = dict(value=1187.64177, ms_per_step=13.4712, roofline=dict(frac=0.30321, bound="hbm", traffic=474.7e6, algorithmic_bytes=217.9e6),
               parity_vs_oracle=dict(rel_l2=8.365e-6), cpu_baseline=dict(value=3.0331))
    res = dict(value=148.2944, ms_per_step=107.9, roofline=dict(frac=0.40569, bound="mfma", traffic=1697262912.0, algorithmic_bytes=1599897600.0,
                                                               mfma_util_pmc_regulariser=0.49905), roofline_fft=dict(frac=0.5477, executed_frac=0.3142),
               parity_vs_oracle=dict(rel_l2=2.0646e-7), cpu_baseline=dict(value=0.1961), exact_fp32_route=dict(value=98.08), streamed_inputs=dict(value=145.7),
               other_configs={k: dict(sub) for k in ("e2evn_6cascade_15coil_640x372", "qcirim_4echo_32coil_256x256", "cirim_training_bf16_15coil_640x372",
                                                     "e2evn_training_15coil_640x372", "cirim_2d_mask_15coil_640x372",
                                                     "cirim_8cascade_x5_time_steps_rimblock_direct")})
    s = bench.summary_of(res)
    assert len(json.dumps(s)) <= 1024, len(json.dumps(s))
    assert s["headline"]["v"] == 148.3 and s["headline"]["traf"] == 1.061 and s["headline"]["mfma_busy_reg"] == 0.499
    assert set(s) == {"headline", "bf16x3", "streamed", "e2evn", "qcirim", "train_bf16", "train_e2evn", "mask2d", "rim5"}
    assert s["e2evn"] == dict(v=1188.0, ms=13.47, frac=0.3032, bound="hbm", traf=2.179, rel=8.365e-06, cpu=3.033)
    res["cpu_baseline"]["sec_per_slice_min"] = 3.2                                         # the fastest CPU slice beside the mean
    assert bench.summary_of(res)["headline"]["cpu_max"] == 0.3125
    src = open(os.path.join(root, "bench.py")).read()
    assert 'res["summary"] = summary_of(res)' in src and src.rindex('res["summary"] = summary_of(res)') > src.index('res["other_configs"] = others')


def test_bench_line_is_short():
    """Round 5's driver record could not parse a 24.9 KB line (19.8 KB had parsed): what bench.py prints is bench.compact_line(res) -- the contract's
    keys, trimmed `roofline` / `cpu_baseline`, one short record per other configuration, `summary` last -- within bench.LINE_LIMIT characters however
    much the full record (written to bench.DETAIL_FILE) grows."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_module3", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert bench.LINE_LIMIT <= 8000
    full = json.load(open(os.path.join(root, "profiles", "r05_v9_bench.json")))            # the 24.9 KB record the driver failed on
    assert len(json.dumps(full)) > 20000
    line = bench.compact_line(full)
    text = json.dumps(line)
    assert len(text) <= bench.LINE_LIMIT, len(text)
    back = json.loads(text)
    assert back == line and list(back)[-1] == "summary"
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in back, k
    assert back["value"] == pytest.approx(full["value"], rel=1e-5) and back["config"]["workload"].startswith("CIRIM 8 cascades")
    rf, cb = back["roofline"], back["cpu_baseline"]
    assert rf["bound"] == "mfma" and rf["unit"] == "TFLOP/s" and rf["frac"] == pytest.approx(rf["achieved"] / rf["peak"], rel=1e-4)
    assert rf["traffic"] > 0 and len(rf["kernel"]) <= 200
    assert cb["kind"] == "port" and cb["cores"] == 16 and cb["value"] > 0 and cb["unit"] == "slices/s" and len(cb["sample"]) <= 220
    assert not any(isinstance(v, (list, dict)) for v in cb.values())
    assert set(back["other_configs"]) == set(full["other_configs"])
    for r in back["other_configs"].values():
        assert r["value"] > 0
    # a record that grows without bound still gives a short line, and the summary survives
    fat = json.loads(json.dumps(full))
    fat["roofline"]["note"] = "x" * 50000
    for r in fat["other_configs"].values():
        r["per_tensor"] = {f"cirim.{i}.layers.0.convs.conv_layer.weight": 0.1 * i for i in range(400)}
        r["config"] = dict(workload="w" * 5000)
    fat["other_configs"].update({f"extra_{i}": dict(fat["other_configs"]["e2evn_6cascade_15coil_640x372"]) for i in range(40)})
    fat["summary"] = bench.summary_of(fat)
    text = json.dumps(bench.compact_line(fat))
    assert len(text) <= bench.LINE_LIMIT or "other_configs" not in json.loads(text)
    assert json.loads(text)["summary"]["headline"]["v"] == pytest.approx(full["value"], rel=1e-3)
    src = open(os.path.join(root, "bench.py")).read()
    assert "print(json.dumps(compact_line(res)), flush=True)" in src and src.count("print(json.dumps(res)") == 0


def test_bench_dump_outputs_is_bounded_and_reproducible(tmp_path):
    """`bench.py --dump-outputs DIR`: the headline's nested output (two streams of list[cascade][time_step] complex images) as float32 .npy files
    under the size limit -- the last leaf (the final image) whole, the others as a seeded sample that is the same from run to run."""
    import importlib.util
    import os
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_module_dump", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    g = torch.Generator().manual_seed(3)

    def outs():
        return [[[torch.randn(2, 40, 30, dtype=torch.complex64, generator=g) for _ in range(3)] for _ in range(2)] for _ in range(2)]

    small = outs()
    bench.write_outputs(str(tmp_path / "a"), small)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(f"out_{c}_{t}.npy" for c in range(2) for t in range(3))
    a = np.load(tmp_path / "a" / "out_1_2.npy")
    assert a.dtype == np.float32 and a.shape == (2, 2, 40, 30, 2)
    assert np.array_equal(a[1], torch.view_as_real(small[1][1][2]).numpy())
    big = outs()
    limit = bench.DUMP_LIMIT_BYTES
    try:
        bench.DUMP_LIMIT_BYTES = 100000                     # smaller than the set (6 leaves of 2 x 2 x 40 x 30 x 8 bytes), larger than twice its last leaf
        bench.write_outputs(str(tmp_path / "b"), big)
        bench.write_outputs(str(tmp_path / "c"), big)
    finally:
        bench.DUMP_LIMIT_BYTES = limit
    total = sum(os.path.getsize(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b"))
    assert total <= 100000
    assert np.array_equal(np.load(tmp_path / "b" / "out_1_2.npy"), torch.view_as_real(torch.stack([o[1][2] for o in big])).numpy())
    s = np.load(tmp_path / "b" / "out_0_0.npy")
    assert s.ndim == 2 and s.shape[1] == 2 and 0 < s.shape[0] < 2 * 2 * 40 * 30
    for f in os.listdir(tmp_path / "b"):
        assert np.array_equal(np.load(tmp_path / "b" / f), np.load(tmp_path / "c" / f)), f


def _fake_kfd(tmp_path, readable_gpus):
    """A KFD topology like the MI355X hosts': two CPU nodes (KFD 0, 1) with four GPUs each as PCIe links (KFD 2-5, 6-9); only `readable_gpus` may be opened."""
    base = tmp_path / "class/kfd/kfd/topology/nodes"
    for c, gpus in ((0, (2, 3, 4, 5)), (1, (6, 7, 8, 9))):
        d = base / str(c)
        (d / "io_links").mkdir(parents=True)
        (d / "properties").write_text("cpu_cores_count 128\nsimd_count 0\nlocation_id 0\n")
        (d / "io_links/0").mkdir()
        (d / "io_links/0/properties").write_text(f"type 1\nnode_from {c}\nnode_to {1 - c}\nweight 32\n")
        for i, g in enumerate(gpus):
            (d / f"io_links/{i + 1}").mkdir()
            (d / f"io_links/{i + 1}/properties").write_text(f"type 2\nnode_from {c}\nnode_to {g}\nweight 20\n")
    for g in range(2, 10):
        d = base / str(g)
        d.mkdir(parents=True)
        if g in readable_gpus:
            (d / "properties").write_text("cpu_cores_count 0\nsimd_count 1024\nlocation_id 1234\n")
        # (a GPU outside the process's device cgroup: the file cannot be read -- here it does not exist)
    for n, cl in ((0, "0-63,128-191"), (1, "64-127,192-255")):
        d = tmp_path / f"devices/system/node/node{n}"
        d.mkdir(parents=True)
        (d / "cpulist").write_text(cl + "\n")
    return str(tmp_path)


def test_rank_binds_itself_to_the_numa_node_of_its_gpu(tmp_path):
    """sharding.bind_rank_to_gpu_numa_node: the KFD topology's PCIe links give the socket of every GPU; the devices a process cannot open are skipped like HIP
    skips them; an explicit device list renumbers; an unreadable topology changes nothing."""
    from mridc_amd import sharding
    root = _fake_kfd(tmp_path / "all", set(range(2, 10)))
    assert sharding.gpu_numa_nodes(root) == [0, 0, 0, 0, 1, 1, 1, 1]
    assert sharding.bind_rank_to_gpu_numa_node(1, root, environ={}, apply=False) == {"node": 0, "cpus": 128}
    assert sharding.bind_rank_to_gpu_numa_node(6, root, environ={}, apply=False) == {"node": 1, "cpus": 128}
    assert sharding.bind_rank_to_gpu_numa_node(0, root, environ={"HIP_VISIBLE_DEVICES": "7,0"}, apply=False) == {"node": 1, "cpus": 128}
    assert sharding.bind_rank_to_gpu_numa_node(0, root, environ={"ROCR_VISIBLE_DEVICES": "GPU-deadbeef"}, apply=False) is None
    assert sharding.bind_rank_to_gpu_numa_node(8, root, environ={}, apply=False) is None
    one = _fake_kfd(tmp_path / "one", {7})                                 # a one-GPU box of the pool: device 0 is KFD node 7, on the second socket
    assert sharding.gpu_numa_nodes(one) == [1]
    assert sharding.bind_rank_to_gpu_numa_node(0, one, environ={}, apply=False) == {"node": 1, "cpus": 128}
    # ROCR_VISIBLE_DEVICES and HIP_VISIBLE_DEVICES compose: HIP's list indexes what ROCR left visible
    assert sharding.bind_rank_to_gpu_numa_node(1, root, environ={"ROCR_VISIBLE_DEVICES": "4,5,0", "HIP_VISIBLE_DEVICES": "1,2"}, apply=False) == {"node": 0, "cpus": 128}
    assert sharding.bind_rank_to_gpu_numa_node(0, root, environ={"ROCR_VISIBLE_DEVICES": "4,5,0", "HIP_VISIBLE_DEVICES": "1,2"}, apply=False) == {"node": 1, "cpus": 128}
    # the GPU's PCI function speaks too (numa_node in sysfs): agreement keeps the answer, a disagreement withdraws it, a memory-only NUMA node is not a socket
    import pathlib
    chk = pathlib.Path(_fake_kfd(tmp_path / "pci", set(range(2, 10))))
    for g in range(2, 10):
        (chk / f"class/kfd/kfd/topology/nodes/{g}/properties").write_text(f"cpu_cores_count 0\nsimd_count 1024\ndomain 0\nlocation_id {(0x10 + g) << 8}\n")
        d = chk / f"bus/pci/devices/0000:{0x10 + g:02x}:00.0"
        d.mkdir(parents=True)
        (d / "numa_node").write_text(("1" if g == 3 else ("-1" if g == 4 else str(0 if g < 6 else 1))) + "\n")
    assert sharding.gpu_numa_nodes(str(chk)) == [0, None, 0, 0, 1, 1, 1, 1]          # GPU 1: PCI says node 1, KFD says node 0 -> no answer; GPU 2: PCI silent (-1)
    assert sharding.bind_rank_to_gpu_numa_node(1, str(chk), environ={}, apply=False) is None
    mem = chk / "devices/system/node/node2"                                            # renumber: node 0 (CPUs), node 1 memory-only, node 2 (CPUs)
    mem.mkdir(parents=True)
    (mem / "cpulist").write_text((chk / "devices/system/node/node1/cpulist").read_text())
    (chk / "devices/system/node/node1/cpulist").write_text("\n")
    for g in range(2, 10):
        (chk / f"bus/pci/devices/0000:{0x10 + g:02x}:00.0/numa_node").write_text(str(0 if g < 6 else 2) + "\n")
    assert sharding.gpu_numa_nodes(str(chk)) == [0, 0, 0, 0, 2, 2, 2, 2]
    assert sharding.gpu_numa_nodes(str(tmp_path / "nothing")) == []
    assert sharding.bind_rank_to_gpu_numa_node(0, str(tmp_path / "nothing"), environ={}) is None
    assert sharding._parse_cpulist("0-3,8,10-11\n") == {0, 1, 2, 3, 8, 10, 11}


def test_inference_precision_context_and_model_plumbing(monkeypatch):
    """`ops.inference_precision` (what VarNet / UNet / qCIRIM wrap their inference forward in when the reference's `trainer.precision` is 16, base_vn_run.yaml:98):
    nests and restores, also on an exception; `resolve_precision16` takes the model's own precision before the process default (MRIDC_AMD_PRECISION) and
    accepts pytorch-lightning's spellings; the models read `trainer.precision` first, then cfg["precision"].  (No GPU call: the kernels behind the switch are
    tests/test_gpu_unet_p16.py.)"""
    import types
    from mridc_amd import ops, synthetic
    from mridc_amd.collections.reconstruction.models.unet import UNet
    from mridc_amd.collections.reconstruction.models.vn import VarNet
    assert not ops._precision16()
    with ops.inference_precision(16):
        assert ops._precision16()
        with ops.inference_precision(None):
            assert not ops._precision16()
        with ops.inference_precision("16-mixed"):
            assert ops._precision16()
        assert ops._precision16()
    assert not ops._precision16()
    with pytest.raises(RuntimeError):
        with ops.inference_precision(16):
            raise RuntimeError("x")
    assert not ops._precision16()
    import threading, time          # the switch is per thread: a model of another precision in another thread does not see it
    seen = {}

    def worker(name, prec, delay):
        with ops.inference_precision(prec):
            time.sleep(delay)
            seen[name] = ops._precision16()
    ts = [threading.Thread(target=worker, args=("a", 16, 0.2)), threading.Thread(target=worker, args=("b", None, 0.05))]
    [t.start() for t in ts], [t.join() for t in ts]
    assert seen == {"a": True, "b": False} and not ops._precision16()
    monkeypatch.delenv("MRIDC_AMD_PRECISION", raising=False)
    assert ops.resolve_precision16(None) is None and ops.resolve_precision16(32) is None and ops.resolve_precision16("bf16") is None
    assert ops.resolve_precision16(16) == 16 and ops.resolve_precision16("16") == 16 and ops.resolve_precision16("16-mixed") == 16
    monkeypatch.setenv("MRIDC_AMD_PRECISION", "16")
    assert ops.resolve_precision16(None) == 16 and ops.resolve_precision16(32) is None            # a stated precision wins over the process default
    monkeypatch.delenv("MRIDC_AMD_PRECISION")
    cfg = dict(synthetic.E2EVN_BASELINE_CFG, num_cascades=1)
    assert VarNet(cfg).precision is None and VarNet(cfg)._inference_precision() is None
    assert VarNet(dict(cfg, precision=16))._inference_precision() == 16
    assert VarNet(dict(cfg, precision=32), trainer=types.SimpleNamespace(precision=16))._inference_precision() == 16      # the trainer first, as in the reference
    assert UNet(cfg, trainer=types.SimpleNamespace(precision="16-mixed")).precision == "16-mixed"
