"""CPU checks of the C-ABI boundary, all in one place: include/t3d.h, the tables the library makes of it (t3d_abi_entry,
t3d_abi_struct), what the library exports, and every Python mirror -- the ctypes argument types, the struct classes and record
dtypes, the enum values, the set of calls a step may contain (no compute calls -- there is no GPU here)."""
import ctypes
import os
import re
import struct

import pytest

from conftest import PKG, ROOT

HEADER = open(os.path.join(ROOT, 'include', 't3d.h')).read()
CODE = re.sub(r'/\*.*?\*/', '', HEADER, flags=re.S)


# ---- the header, read independently of the binding ----------------------------------------------------------------------------------
def _declarations():
    """{name: [argument text, ...]} of every `int t3d_*(...);` of the header."""
    out = {}
    for name, args in re.findall(r'\bint\s+(t3d_\w+)\s*\(([^()]*)\)\s*;', CODE):
        assert name not in out, f'{name} is declared twice'
        args = ' '.join(args.split())
        out[name] = [] if args in ('', 'void') else [a.strip() for a in args.split(',')]
    return out


STRUCT_ARGS = {'t3d_prologue': 'Prologue', 't3d_bnbwd': 'BnBwd', 't3d_loss_cfg': 'LossCfg', 't3d_draw_style': 'DrawStyleC'}
SCALARS = {'int': ctypes.c_int, 'long long': ctypes.c_longlong, 'unsigned long long': ctypes.c_ulonglong,
           'float': ctypes.c_float, 'double': ctypes.c_double}


def _classify(arg, N):
    """The ctypes type of one argument from its declaration TEXT -- the only check on the letter mapping of csrc/abi.hip and on
    `_native._ARGTYPE`, so it decides by the text alone (the binding's struct classes are only what it answers with).
    None: the text is not understood."""
    m = re.fullmatch(r'((?:const\s+)?(?:unsigned\s+)?[a-z_0-9]+(?:\s+long)?)((?:\s*\*\s*(?:const\s*)?)*)\s*(\w+)', arg)
    if not m:
        return None
    base, stars = re.sub(r'^const\s+', '', m.group(1)), m.group(2).count('*')
    if stars:
        # a pointer to a struct that Python passes as a ctypes.Structure; t3d_bn_fold descriptors are DEVICE addresses
        return ctypes.POINTER(getattr(N, STRUCT_ARGS[base])) if base in STRUCT_ARGS and stars == 1 else ctypes.c_void_p
    return SCALARS.get(base)


def _enums():
    """{T3D_NAME: value} of every `enum { ... }` and every `#define T3D_NAME <integer>` of the header."""
    out = {}
    for body in re.findall(r'\benum\s*\{([^}]*)\}', CODE):
        for name, val in re.findall(r'(T3D_\w+)\s*=\s*(-?(?:0x[0-9a-fA-F]+|\d+))', body):
            assert name not in out
            out[name] = int(val, 0)
        assert len(re.findall(r'T3D_\w+', body)) == body.count('='), f'an enumerator without a value: {body}'
    for name, val in re.findall(r'^#define\s+(T3D_\w+)\s+(-?(?:0x[0-9a-fA-F]+|\d+))\s*$', CODE, flags=re.M):
        assert name not in out
        out[name] = int(val, 0)
    return out


def _header_structs():
    """{t3d_name: ([member names in order], N of a trailing `/* N bytes */` or None)}."""
    out = {}
    for body, name, size in re.findall(r'typedef struct \{([^}]*)\}\s*(t3d_\w+);(?:[ \t]*/\*\s*(\d+) bytes\s*\*/)?', HEADER):
        names = []
        for decl in re.sub(r'/\*.*?\*/', '', body, flags=re.S).split(';'):
            names += [re.search(r'(\w+)\s*(?:\[\w+\]\s*)*$', d).group(1) for d in decl.split(',') if d.strip()]
        out[name] = (names, int(size) if size else None)
    return out


def _exported(path):
    """Names of the functions an ELF64 shared object defines and exports (.dynsym)."""
    b = open(path, 'rb').read()
    assert b[:6] == b'\x7fELF\x02\x01', 'not a little-endian ELF64 file'
    shoff, = struct.unpack_from('<Q', b, 0x28)
    shentsize, shnum = struct.unpack_from('<HH', b, 0x3A)
    sections = [struct.unpack_from('<IIQQQQIIQQ', b, shoff + i * shentsize) for i in range(shnum)]
    names = set()
    for _, kind, _, _, off, size, link, _, _, entsize in sections:
        if kind != 11:                      # SHT_DYNSYM
            continue
        stroff = sections[link][4]
        for o in range(off, off + size, entsize):
            st_name, st_info, _, st_shndx = struct.unpack_from('<IBBH', b, o)
            if st_shndx and st_info & 15 == 2 and st_info >> 4 in (1, 2):       # defined, a function, global or weak
                names.add(b[stroff + st_name:b.index(b'\0', stroff + st_name)].decode())
    return names


@pytest.fixture(scope='module')
def N():
    from torchdet3d import _native
    assert os.path.exists(_native.LIB_PATH), 'run `python __graft_entry__.py` (build()) first'
    return _native


# ---- 1. names ------------------------------------------------------------------------------------------------------------------------
def test_library_exports_every_declared_symbol(N):
    names = sorted(_declarations())
    assert len(names) == len(set(re.findall(r'\bint\s+(t3d_\w+)\s*\(', CODE))) >= 123, 'a declaration the parser does not read'
    lib = ctypes.CDLL(N.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f'{n} declared in include/t3d.h but not exported'
    assert sorted(N.SIGNATURES) == names, 'the library\'s table (csrc/abi_entries.h) and include/t3d.h disagree'
    assert sorted(n for n in _exported(N.LIB_PATH) if n.startswith('t3d_')) == names, 'exported but not declared, or the reverse'


def test_version_call(N):
    assert N.lib().t3d_version() >= 1


def test_the_tables_end_with_an_argument_error(N):
    lib, name = N.lib(), ctypes.c_char_p()
    for fn, rows in ((lib.t3d_abi_entry, len(N.SIGNATURES)), (lib.t3d_abi_struct, len(N.abi_structs()))):
        assert fn(rows - 1, ctypes.byref(name), None, None) == 0 and name.value.startswith(b't3d_')
        assert fn(rows - 1, None, None, None) == 0                       # every output is optional
        assert fn(rows, ctypes.byref(name), None, None) == N.ERR_ARG and fn(-1, None, None, None) == N.ERR_ARG


# ---- 2. types ------------------------------------------------------------------------------------------------------------------------
def test_every_argument_type_is_the_headers(N):
    decls = _declarations()
    want = {name: [_classify(a, N) for a in args] for name, args in decls.items()}
    skipped = [(n, a) for n, args in decls.items() for a, t in zip(args, want[n]) if t is None]
    assert not skipped, f'declarations the classifier does not read: {skipped}'
    wrong = {n: (decls[n], N.SIGNATURES[n]) for n in decls if N.SIGNATURES[n] != want[n]}
    assert not wrong, wrong
    for n in decls:
        fn = getattr(N.lib(), n)
        assert list(fn.argtypes) == want[n] and fn.restype is ctypes.c_int, n
    # the classifier tells the cases apart (it is the only witness): one known answer per code
    assert want['t3d_dropout_mask'] == [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_ulonglong, ctypes.c_float,
                                        ctypes.c_void_p]
    assert want['t3d_set_reduction_replicas'] == [ctypes.c_int, ctypes.c_longlong]
    assert want['t3d_bn_finalize'][2] is ctypes.c_double and want['t3d_fold_request'] == [ctypes.c_void_p] * 2
    assert want['t3d_pwconv_dgrad'][3] is N._BP and want['t3d_pwconv_dgrad'][6] is N._PP and want['t3d_loss_fwd_bwd'][0] is N._LP
    assert want['t3d_draw_overlays_u8'][12] is ctypes.POINTER(N.DrawStyleC) and want['t3d_version'] == []
    assert want['t3d_ssd_multibox_loss'][2] is ctypes.c_void_p and len(want['t3d_ssd_multibox_loss']) == 29
    assert (N._I, N._L, N._F, N._D, N._P) == (ctypes.c_int, ctypes.c_longlong, ctypes.c_float, ctypes.c_double, ctypes.c_void_p)


# ---- 3. structs ----------------------------------------------------------------------------------------------------------------------
def _ctypes_layout(cls):
    return ctypes.sizeof(cls), [(n, getattr(cls, n).offset, getattr(cls, n).size) for n, _ in cls._fields_]


def _dtype_layout(dt):
    return dt.itemsize, [(n, dt.fields[n][1], dt.fields[n][0].itemsize) for n in dt.names]


def _mirrors(N):
    from torchdet3d.dataloaders import detection, jpeg, objectron
    return {'t3d_prologue': _ctypes_layout(N.Prologue), 't3d_bnbwd': _ctypes_layout(N.BnBwd), 't3d_loss_cfg': _ctypes_layout(N.LossCfg),
            't3d_bn_fold': _ctypes_layout(N.BnFold), 't3d_draw_style': _ctypes_layout(N.DrawStyleC),
            't3d_aug_sample': _dtype_layout(objectron.AUG_SAMPLE_DTYPE), 't3d_aug_chain': _dtype_layout(objectron.AUG_CHAIN_DTYPE),
            't3d_det_sample': _dtype_layout(detection.DET_SAMPLE_DTYPE), 't3d_jpeg_info': _dtype_layout(jpeg.INFO_DTYPE),
            't3d_jpeg_seg': _dtype_layout(jpeg.SEG_DTYPE), 't3d_jpeg_item': _dtype_layout(jpeg.ITEM_DTYPE)}


SIZES = {'t3d_aug_sample': 80, 't3d_aug_chain': 280, 't3d_det_sample': 80, 't3d_draw_style': 44, 't3d_jpeg_info': 864,
         't3d_jpeg_seg': 16, 't3d_jpeg_item': 48}


def test_every_struct_of_the_header_is_in_the_table_member_for_member(N):
    table, header = N.abi_structs(), _header_structs()
    assert sorted(table) == sorted(header) and len(table) >= 11
    for name, (members, commented) in header.items():
        size, fields = table[name]
        assert [f for f, _, _ in fields] == members, name
        assert commented in (None, size), f'{name}: the header says {commented} bytes, the compiler {size}'
        assert size == SIZES.get(name, size), name
        end = 0
        for f, off, nbytes in fields:
            assert off >= end and nbytes > 0, (name, f)
            end = off + nbytes
        assert end <= size
    assert {n for n, (_, c) in header.items() if c} == set(SIZES) - {'t3d_draw_style'}


@pytest.mark.parametrize('name', ['t3d_prologue', 't3d_bnbwd', 't3d_loss_cfg', 't3d_bn_fold', 't3d_draw_style', 't3d_aug_sample',
                                  't3d_aug_chain', 't3d_det_sample', 't3d_jpeg_info', 't3d_jpeg_seg', 't3d_jpeg_item'])
def test_python_mirror_has_the_compilers_layout(N, name):
    """Size and, member by member, name, offset and byte extent (an array member is one field on both sides)."""
    size, fields = _mirrors(N)[name]
    assert (size, fields) == N.abi_structs()[name]
    assert size == SIZES.get(name, size)


def test_every_struct_of_the_table_has_a_python_mirror(N):
    assert sorted(_mirrors(N)) == sorted(N.abi_structs())


# ---- 4. constants --------------------------------------------------------------------------------------------------------------------
def test_python_constants_equal_the_headers(N):
    from torchdet3d.dataloaders import detection as D
    from torchdet3d.dataloaders import jpeg as J
    from torchdet3d.dataloaders import objectron as O
    H = _enums()
    mirrors = dict(
        T3D_F32=N.F32, T3D_BF16=N.BF16, T3D_F16=N.F16, T3D_W_FRAG=N.W_FRAG,
        T3D_ACT_NONE=N.ACT['none'], T3D_ACT_RELU=N.ACT['relu'], T3D_ACT_RELU6=N.ACT['relu6'], T3D_ACT_HSWISH=N.ACT['hswish'],
        T3D_OK=0, T3D_ERR_ARG=N.ERR_ARG, T3D_ERR_UNSUPPORTED=N.ERR_UNSUPPORTED,
        T3D_POOL_AVG=N.POOL['avg'], T3D_POOL_MAX=N.POOL['max'], T3D_POOL_AVGMAX=N.POOL['avg+max'],
        T3D_DW_AUTO=N.DW_AUTO, T3D_DW_TILE=N.DW_TILE, T3D_DW_ROW3=N.DW_ROW3, T3D_DW_PLANE7=N.DW_PLANE7, T3D_DW_ROWK=N.DW_ROWK,
        T3D_DW_LDS=N.DW_LDS,
        T3D_PW_AUTO=N.PW_AUTO, T3D_PW_DEEP=N.PW_DEEP, T3D_PW_STREAM=N.PW_STREAM, T3D_PW_REG32=N.PW_REG32, T3D_PW_LDS=N.PW_LDS,
        T3D_PW_TR=N.PW_TR, T3D_PW_PAIR=N.PW_PAIR,
        T3D_PW_OP_FWD=N.PW_OP_FWD, T3D_PW_OP_FWD_STATS=N.PW_OP_FWD_STATS, T3D_PW_OP_MAT=N.PW_OP_MAT, T3D_PW_OP_DGRAD=N.PW_OP_DGRAD,
        T3D_PW_OP_WGRAD=N.PW_OP_WGRAD,
        T3D_DRAW_IDS=N.DRAW_IDS,
        T3D_AUG_FLIP=O.AUG_FLIP, T3D_AUG_LUT=O.AUG_LUT, T3D_AUG_ROTATE=O.AUG_ROTATE, T3D_AUG_SWAP_RB=O.AUG_SWAP_RB,
        T3D_CHAIN_LUT=O.CHAIN_LUT, T3D_CHAIN_HSV=O.CHAIN_HSV, T3D_CHAIN_BRIGHTNESS=O.CHAIN_BRIGHTNESS,
        T3D_CHAIN_CONTRAST=O.CHAIN_CONTRAST, T3D_CHAIN_SATURATION=O.CHAIN_SATURATION, T3D_CHAIN_HUE=O.CHAIN_HUE,
        T3D_CHAIN_WARP2=O.CHAIN_WARP2, T3D_CHAIN_MAX_OPS=O.CHAIN_MAX_OPS,
        T3D_STAGE_MEAN=O.STAGE_MEAN, T3D_STAGE_WARP=O.STAGE_WARP, T3D_STAGE_WARP2=O.STAGE_WARP2,
        T3D_DET_FLIP=D.DET_FLIP, T3D_DET_BRIGHTNESS=D.DET_BRIGHTNESS, T3D_DET_CONTRAST=D.DET_CONTRAST,
        T3D_DET_CONTRAST_LAST=D.DET_CONTRAST_LAST, T3D_DET_HSV=D.DET_HSV, T3D_DET_SATURATION=D.DET_SATURATION, T3D_DET_HUE=D.DET_HUE)
    assert {k: H[k] for k in mirrors} == mirrors
    # T3D_JPEG_*: the loader indexes its blocks-per-MCU table by the sampling code and words every reason the indexer can give
    assert (H['T3D_JPEG_GRAY'], H['T3D_JPEG_444'], H['T3D_JPEG_420']) == (0, 1, 2) and J._BLOCKS_PER_MCU == (1, 3, 6)
    assert sorted(J.REASONS) == sorted([-1] + [v for k, v in H.items() if k.startswith('T3D_JPEG_REASON_')])
    # nothing the header defines is left without a mirror, except T3D_ERR_LAUNCH: Python only ever reports that code as a number
    assert set(H) - set(mirrors) - {k for k in H if k.startswith('T3D_JPEG_')} == {'T3D_ERR_LAUNCH'}


# ---- 5. the calls a step may contain --------------------------------------------------------------------------------------------------
STEP_ENTRIES = '''
    t3d_dwconv_fwd t3d_bn_finalize t3d_bn_eval_affine t3d_bn_eval_affine_batched t3d_pwconv_fwd t3d_pwconv_dgrad t3d_pack_weight
    t3d_set_dw_slots t3d_set_exact_pool t3d_sum_slots_batched t3d_dwconv_bwd t3d_pwconv_wgrad t3d_pwconv_yfree_prep
    t3d_pwconv_dgrad_yfree t3d_pwconv_wgrad_yfree t3d_pwconv_yfree_prep2 t3d_pwconv_bwd_yfree t3d_pwconv_bwd_yfree_w
    t3d_pwconv_wgrad_yfree_finish t3d_bn_bwd_finalize t3d_stem_im2col t3d_stem_im2col_u8 t3d_crop_resize_u8 t3d_pwconv_fwd_mat
    t3d_im2col t3d_im2col_nchw t3d_col2im_bwd t3d_pack_conv_weight t3d_unpack_conv_grad t3d_maxpool_fwd t3d_maxpool_bwd
    t3d_res_relu_fwd t3d_res_relu_bwd t3d_subsample t3d_ir_block_eval t3d_bn_apply t3d_bn_act_bwd t3d_gap_fwd t3d_pool_fwd
    t3d_pool_bwd t3d_head_fwd t3d_linear_fwd t3d_head_fwd_all t3d_head_bwd t3d_head_bwd_weights t3d_se_fwd_fused t3d_se_bwd_data
    t3d_se_bwd_weights t3d_se_after_sums t3d_se_after_apply t3d_se_after_bwd t3d_set_reduction_replicas t3d_set_workspace
    t3d_set_main_workspace t3d_fold_request t3d_pack_weights_batched t3d_pwconv_pack_frag t3d_adamw_step t3d_set_grad_watch
    t3d_sgd_step t3d_rmsprop_step t3d_adadelta_step t3d_zero_batched t3d_copy_cols t3d_bn_bias_grad t3d_se_bwd_affine
    t3d_dropout_mask t3d_loss_fwd_bwd t3d_metrics_per_sample t3d_iou3d t3d_box_iou3d t3d_ssd_decode_nms t3d_expdw_fwd
    t3d_track_step t3d_ssd_select_rects t3d_head_select t3d_track_kp_to_frame t3d_objectron_pairs t3d_objectron_hitmiss
    t3d_draw_overlays_u8 t3d_ssd_multibox_loss t3d_ssd_head_bwd t3d_ssd_cap_per_image t3d_coco_match'''.split()


def test_a_plan_takes_exactly_the_step_entries(N):
    """The flagged rows of the table are the set a plan could record before the table existed; `t3d_plan_add_call` takes each of
    them with the table's arity (one argument fewer is an argument error, not 'unsupported'), refuses every other entry point
    as unsupported, and a refused call adds no op.  (t3d_plan_create / _add_call / _destroy make no HIP call.)"""
    assert len(STEP_ENTRIES) == len(set(STEP_ENTRIES)) == 84
    assert sorted(N.STEP_ENTRIES) == sorted(STEP_ENTRIES)
    lib, plan = N.lib(), ctypes.c_void_p()
    assert lib.t3d_plan_create(ctypes.byref(plan)) == 0
    try:
        for name, types in sorted(N.SIGNATURES.items()):
            n = len(types)
            kinds, words, sizes = (ctypes.c_int * n)(), (ctypes.c_ulonglong * n)(), (ctypes.c_int * n)()
            rc = lib.t3d_plan_add_call(plan, name.encode(), n, kinds, words, sizes)
            if name in N.STEP_ENTRIES:
                assert rc == 0, name
                assert n >= 1 and lib.t3d_plan_add_call(plan, name.encode(), n - 1, kinds, words, sizes) == N.ERR_ARG, name
            else:
                assert rc == N.ERR_UNSUPPORTED, name
        assert lib.t3d_plan_add_call(plan, b't3d_no_such_entry', 0, None, None, None) == N.ERR_UNSUPPORTED
        assert lib.t3d_plan_num_ops(plan, 0) == lib.t3d_plan_num_ops(plan, -1) == 84
    finally:
        lib.t3d_plan_destroy(plan)


def test_plan_source_lists_no_entry_names():
    """csrc/plan.hip takes its table from csrc/abi_entries.h; the binding keeps no signature table of its own."""
    plan = open(os.path.join(PKG, 'csrc', 'plan.hip')).read()
    assert 'T3D_ABI_ENTRIES(' in plan and not re.findall(r'T3D_E\(t3d_', plan)
    assert 'SIGNATURES = {' not in open(os.path.join(PKG, 'torchdet3d', '_native.py')).read()


def test_every_kernel_launch_goes_through_the_launch_macro():
    """csrc/common.h, the rule next to T3D_LAUNCH: a replayed fork waits for the last kernel a call launched through the macro,
    so no source may launch a kernel any other way, and an async memset inside an entry point must be followed by a kernel
    launch of the same entry point (in-order stream: that kernel's completion covers it)."""
    csrc = os.path.join(ROOT, '3d-object-detection.pytorch_amd', 'csrc')
    for f in sorted(os.listdir(csrc)):
        if not f.endswith(('.hip', '.h')):
            continue
        lines = open(os.path.join(csrc, f)).read().split('\n')
        code = [re.sub(r'//.*', '', ln) for ln in lines]
        for i, ln in enumerate(code):
            if f != 'common.h':
                assert 'hipLaunchKernelGGL' not in ln and '<<<' not in ln, f'{f}:{i + 1}: raw kernel launch'
            if 'hipMemsetAsync' in ln and f != 'plan.hip':
                rest = code[i + 1:i + 60]
                upto = next((j for j, r in enumerate(rest) if re.match(r'^(extern "C" )?\w[\w \*]*\(.*\{\s*$', r) or r.startswith('}')), len(rest))
                assert any('T3D_LAUNCH' in r for r in rest[:upto]), f'{f}:{i + 1}: a memset that is not followed by a kernel launch'
