"""GPU parity tests (-m gpu): the gfx950 library through the C ABI vs plain torch fp32, at the real
attention-site / resnet shapes of SD-1.5 plus ragged edge cases."""
import os

import pytest
import torch

from controllora_amd import kernels as K
from tests import kernel_cases as KC

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True, scope="module")
def _native_lib_loaded():
    from controllora_amd import capi
    L = capi.lib()
    assert L.require_device and L.path.endswith("libclora.so")
    yield


@pytest.mark.parametrize("M,N,K,split", [(300, 72, 96, 1), (4096, 960, 320, 1), (1024, 1280, 1280, 1), (256, 1280, 1280, 4),
                                         (308, 640, 768, 1), (4096, 2560, 320, 1), (1024, 320, 1280, 2), (64, 8, 40, 1),
                                         # M * N / 8 just past 2048 blocks x 256: the second trip of splitk_finish_kernel's grid-stride loop alone
                                         (4104, 1032, 64, 2), (4104, 1032, 64, 3)])
def test_gemm_plain(M, N, K, split):
    KC.case_gemm_plain(DEV, M, N, K, split)


@pytest.mark.parametrize("split", [1, 2])
def test_gemm_epilogue(split):
    KC.case_gemm_epilogue(DEV, M=2000, N=320, K_=320, split_k=split)


@pytest.mark.parametrize("kw", [dict(stride=1, pad=1), dict(stride=2, pad=1), dict(asym=True, stride=2, pad=0), dict(ups=True)])
def test_conv_fwd_dgrad_wgrad(kw):
    KC.case_conv(DEV, 2, 32, 32, 64, 128, **kw)


def test_conv_unet_shape():
    KC.case_conv(DEV, 1, 32, 32, 320, 640)


@pytest.mark.parametrize("Bn,H,W,Ci,Co", [(4, 512, 512, 32, 32), (4, 256, 256, 32, 64), (4, 128, 128, 64, 64), (2, 37, 192, 64, 64), (1, 5, 128, 32, 16)])
def test_conv_wgrad_patch_kernel(Bn, H, W, Ci, Co):
    KC.case_conv_wgrad_patch(DEV, Bn, H, W, Ci, Co)


@pytest.mark.parametrize("Bn,H,W,Ci,Co", [(4, 512, 512, 32, 32), (4, 256, 256, 64, 64), (2, 38, 384, 32, 64), (1, 6, 128, 64, 24)])
def test_conv_wgrad_patch_kernel_stride2(Bn, H, W, Ci, Co):
    """the downsamplers (reference models.py SimpleDownEncoderBlock2D: F.pad(0, 1, 0, 1) + 3x3 stride 2); H, W = INPUT size"""
    KC.case_conv_wgrad_patch(DEV, Bn, H, W, Ci, Co, stride=2)


@pytest.mark.parametrize("Bn,H,W,Ci,Co", [(4, 512, 512, 32, 32), (4, 256, 256, 32, 64), (2, 37, 384, 64, 32), (1, 5, 128, 32, 24), (4, 512, 512, 8, 32), (1, 6, 256, 8, 64),
                                          # H = 17: row chunks of 8, 8 and 1 (KC.case_conv_strip), the shapes of the CPU suite
                                          (1, 17, 128, 32, 32), (2, 17, 128, 64, 32), (1, 17, 256, 32, 64), (2, 17, 128, 8, 32), (1, 17, 256, 32, 8),
                                          (1, 17, 128, 8, 64)])
def test_conv_strip_kernel(Bn, H, W, Ci, Co):
    KC.case_conv_strip(DEV, Bn, H, W, Ci, Co)


def test_conv_small_channels():
    KC.case_conv(DEV, 1, 64, 64, 8, 32)


@pytest.mark.parametrize("shapes", [((232, 256, 256),), ((229, 253, 256), (16, 3, 8), (64, 32, 32))])
def test_conv_weight_pack_and_wgrad_unpack_past_their_caps(shapes):
    """Co * 9 * Cip = 534,528 / 527,616 > 2048 x 256 (1024 x 256 in the multi-job forms); padded input (253 -> 256) and output (229 -> 232)
    channels; one multi-job launch whose jobs differ in size"""
    KC.case_conv_pack_unpack_past_cap(DEV, shapes)


@pytest.mark.parametrize("Co", [72, 136])
def test_conv_wgrad_gather_kernel_several_channel_tiles(Co):
    """conv_wgrad_kernel (16 input channels: never the patch kernel) with two and three 64-wide output-channel tiles, the last one
    ragged (8 channels): dW with and without the bias column, conv_wgrad_into and conv_wgrad_staged under the elementwise limit"""
    KC.case_conv(DEV, 1, 8, 8, 16, Co)


@pytest.mark.parametrize("tile", [72, 76])
def test_conv_patch_kernel_uneven_split(tile):
    """192 channels = three 64-channel slabs: split-K 2 gives 2 + 1 slabs, the second split's range is clamped to the slab count (the
    other CPU shapes have one or two slabs, which every split count divides: tests/test_kernel_mutants_emu.py patch_clamp)"""
    KC.case_conv_patch(DEV, 1, 8, 8, 192, 64, tile)


@pytest.mark.parametrize("tile", KC.ALL_TILE_CFGS)
def test_gemm_tile_configs(tile):
    """every main-loop variant (tile shape x ring depth), with ragged M/N/K, split-K and the fused epilogue"""
    KC.case_gemm_plain(DEV, 1000, 328, 1256, 1, tile_cfg=tile)
    KC.case_gemm_plain(DEV, 333, 640, 2568, 3, tile_cfg=tile)
    KC.case_gemm_epilogue(DEV, M=2000, N=320, K_=320, split_k=1, tile_cfg=tile)
    KC.case_conv(DEV, 2, 32, 32, 64, 128, tile_cfg=tile)
    KC.case_conv(DEV, 1, 32, 32, 320, 320, tile_cfg=tile)          # Cin % 64 == 0: the BK = 64 variants take the fast tap walk


@pytest.mark.parametrize("M,N,K,split", [(4096, 2560, 320, 1), (1000, 520, 1096, 2), (16384, 1280, 320, 1), (513, 264, 8200, 1), (2048, 2048, 2048, 1)])
def test_gemm_eight_phase_tile(M, N, K, split):
    """tile_cfg 59 (gemm_8p_kernel: 256x256 tile, two wave rows one barrier apart, half-tile LDS-DMA seven ahead): the level-0
    FeedForward shapes, ragged M / N / K tail, split-K, a long K; elementwise outlier guard, the derived elementwise limit (fp64 reference) and repeat-launch bit equality inside
    the case (a rare early read of a staged buffer would show as a few wrong tiles)"""
    import math
    import torch
    from controllora_amd import kernels as K_
    g = torch.Generator().manual_seed(M + K)
    A, B = KC.rnd((M, K), DEV, g), KC.rnd((N, K), DEV, g, 1 / math.sqrt(K))
    ref, mag = KC.d64(A) @ KC.d64(B).T, KC.d64(A).abs() @ KC.d64(B).abs().T
    first = None
    for _ in range(4):
        out = K_.gemm(A, B, M, N, K, split_k=split, tile_cfg=59, _tuned=False)
        assert KC.rel(out, ref) < 6e-4
        KC.no_outliers(out, ref)
        KC.within_limit(out, ref, mag, K + split, what=f"gemm_eight_phase: {(M, N, K, split)}")
        if first is None:
            first = out.clone()
        assert torch.equal(out, first)


@pytest.mark.parametrize("tile", [71, 72, 73, 74, 75, 76, 79])  # 79 = 256x160 (64x80 wave tiles, all 160 KB of LDS): first hardware run in round 5
@pytest.mark.parametrize("Bn,H,W,Ci,Co", [(4, 64, 64, 320, 320), (4, 32, 32, 640, 640), (2, 16, 16, 1280, 640), (4, 8, 8, 1280, 1280),
                                          (1, 32, 32, 320, 320), (3, 8, 8, 128, 72)])
def test_conv_patch_kernel(tile, Bn, H, W, Ci, Co):
    """patch-staged 3x3 conv at the ResnetBlock2D shapes of every UNet level (forward, dgrad, split-K, fused epilogue)"""
    KC.case_conv_patch(DEV, Bn, H, W, Ci, Co, tile)


@pytest.mark.parametrize("tile", [71, 72, 76])
@pytest.mark.parametrize("Bn,H,Ci", [(2, 32, 640), (2, 16, 1280), (1, 8, 1280)])
def test_conv_patch_kernel_upsampled(tile, Bn, H, Ci):
    KC.case_conv_patch_upsampled(DEV, Bn, H, H, Ci, Ci, tile)


@pytest.mark.parametrize("tile", [77, 78])
@pytest.mark.parametrize("Bn,H,W,Ci,Co", [(1, 512, 512, 128, 128), (2, 256, 256, 256, 256), (2, 128, 128, 512, 512), (1, 256, 256, 128, 256)])
def test_conv_patch_kernel_row_segments_vae_shapes(tile, Bn, H, W, Ci, Co):
    """tile_cfg 77 / 78 (392-pixel patch, one 128-pixel row or row segment per tile) at the SD-1.5 VAE's level shapes"""
    KC.case_conv_patch(DEV, Bn, H, W, Ci, Co, tile, fwd_only=True)


@pytest.mark.parametrize("kw", [dict(M=16384, N=320, K_=320, tile_cfg=55), dict(M=16384, N=320, K_=320, tile_cfg=52, t_in_rows=0),
                                dict(M=16384, N=320, K_=320, tile_cfg=54, t_in_rows=4096), dict(M=16384, N=320, K_=320, tile_cfg=51, u_tr=True, bias=False),
                                dict(M=16384, N=960, K_=320, nseg=3, tile_cfg=0, t_in_rows=0), dict(M=32768, N=960, K_=320, nseg=3, tile_cfg=0, t_in_rows=4096),
                                dict(M=4096, N=640, K_=640, tile_cfg=0, t_in_rows=0), dict(M=1024, N=1280, K_=1280, tile_cfg=0, u_tr=True, residual=False),
                                dict(M=4099, N=1920, K_=640, nseg=3, tile_cfg=55, t_in_rows=0), dict(M=131072, N=320, K_=320, tile_cfg=0, t_in_rows=4096),
                                dict(M=4096, N=640, K_=640, tile_cfg=43, t_in_rows=0), dict(M=1024, N=1280, K_=1280, tile_cfg=43, u_tr=True, residual=False),
                                dict(M=4096, N=640, K_=640, tile_cfg=42), dict(M=256, N=1280, K_=1280, tile_cfg=23, t_in_rows=64),
                                dict(M=308, N=1280, K_=768, nseg=2, tile_cfg=43), dict(M=2048, N=1280, K_=1280, tile_cfg=22, u_tr=True, bias=False),
                                dict(M=1024, N=1280, K_=1280, tile_cfg=21, t_in_rows=0), dict(M=8192, N=640, K_=640, tile_cfg=41),
                                dict(M=4096, N=640, K_=640, tile_cfg=26)])
def test_gemm_with_adapter_down_projection_in_the_launch(kw):
    """clora_epilogue_t.lora_dpack at the projection shapes of the step (level 0 q | k | v, out, cross-attention q; the deeper
    levels; the batch-8 and batch-32 row counts; ragged M): T written == A . D^T, output == the unfused formula elementwise,
    repeat launches bit-identical (reference models.py:232-282)"""
    e = KC.case_gemm_fused_down(DEV, **kw)
    print("FUSED_DOWN", kw, f"T rel {e:.2e}")


@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4, 5, 6, 7, 8, 21, 22, 23, 26, 31, 32, 33, 41, 42, 43, 51, 52, 53, 54, 55, 56, 57, 58])
def test_gemm_epilogue_without_rowadd(tile):
    """projection epilogues at real shapes (M = 16384 x N = 320 / 960, ragged variants): two-phase chunk loop of the 8-wave tiles"""
    KC.case_gemm_epilogue_no_rowadd(DEV, M=16384, N=320, K_=320, tile_cfg=tile)
    KC.case_gemm_epilogue_no_rowadd(DEV, M=4100, N=960, K_=320, tile_cfg=tile)
    KC.case_gemm_epilogue_no_rowadd(DEV, M=1000, N=1296, K_=1280, tile_cfg=tile, split_k=2 if tile else 0)


@pytest.mark.parametrize("order", ["n", "auto", "grid"])
@pytest.mark.parametrize("tile", [21, 43, 53, 58, 72, 76])
def test_tile_order_does_not_change_results(tile, order):
    """clora_set_option("tile_order"): which XCD computes which tile is a permutation -- bit-identical GEMM / conv outputs"""
    KC.case_tile_order(DEV, tile, order)


@pytest.mark.parametrize("B,H,Nq,Nk,D", [(2, 8, 4096, 4096, 40), (2, 8, 1024, 77, 80), (3, 5, 300, 300, 160)])
def test_attention_block_order_does_not_change_results(B, H, Nq, Nk, D):
    KC.case_attention_block_order(DEV, B, H, Nq, Nk, D)


@pytest.mark.parametrize("B,H,Nq,Nk,D,fused", [
    (1, 8, 4096, 4096, 40, True), (2, 8, 4096, 77, 40, False), (2, 8, 1024, 1024, 80, True), (2, 8, 1024, 77, 80, False),
    (2, 8, 256, 256, 160, True), (2, 8, 64, 77, 160, False), (1, 2, 70, 70, 40, True), (1, 1, 150, 77, 64, False),
    (1, 2, 20, 20, 8, False)])
def test_attention(B, H, Nq, Nk, D, fused):
    KC.case_attention(DEV, B, H, Nq, Nk, D, fused_qkv=fused)


@pytest.mark.parametrize("Nq,Nk,D", [(4096, 4096, 40), (300, 64, 40), (300, 77, 64), (1024, 1024, 80), (256, 256, 160)])
def test_attention_first_tile_far_below_zero(Nq, Nk, D):
    """first KV tile with every logit below -88: finite outputs, ordinary softmax over the later tiles"""
    KC.case_attention_negative_logits(DEV, 2, 8, Nq, Nk, D)


@pytest.mark.parametrize("Nq,Nk,D", [(1024, 4096, 40), (300, 1000, 80), (70, 300, 160)])
def test_attention_rising_maxima(Nq, Nk, D):
    """forward: lazy exponent reference, rebased on later KV tiles for a subset of the queries (D = 40: rowsum from the ones column)"""
    KC.case_attention(DEV, 2, 8, Nq, Nk, D, ramp=4.0, tol=3e-3)


@pytest.mark.parametrize("B,HW,C,G,silu,train", [(2, 4096, 320, 32, True, False), (2, 1024, 960, 32, True, False),
                                                 (1, 64, 2560, 32, True, False), (2, 4096, 32, 32, True, True),
                                                 (1, 1024, 640, 32, False, False), (1, 37, 64, 8, False, True),
                                                 (4, 256, 1280, 32, True, True), (4, 1024, 1920, 32, True, False),
                                                 (4, 256, 1280, 32, True, False), (4, 64, 2560, 32, False, False), (4, 256, 640, 32, True, False),
                                                 # the UNet's one-launch shapes (bs 4 / 8 / inference batch 32) + ragged row counts
                                                 (4, 64, 1280, 32, True, False), (4, 256, 2560, 32, True, False), (4, 256, 1920, 32, True, False),
                                                 (8, 1024, 640, 32, True, False), (4, 1024, 1280, 32, True, False), (32, 256, 1280, 32, True, False),
                                                 (2, 1000, 640, 32, False, False), (3, 130, 1920, 32, True, False),
                                                 # team plan: the train step's 64x64 / 32x32 maps (bs 4, bs 8), batch 1 / 2, ragged rows
                                                 (4, 4096, 320, 32, True, False), (4, 4096, 640, 32, True, False), (4, 4096, 960, 32, True, False),
                                                 (4, 1024, 320, 32, True, False), (4, 1024, 960, 32, True, False), (8, 4096, 320, 32, True, False),
                                                 (1, 4096, 320, 32, False, False), (2, 1500, 640, 32, True, False),
                                                 # trainable affine, 2 x 36 row chunks (the last one ragged): 72 per-channel partials, the
                                                 # eight-loads-in-flight loop of the dgamma / dbeta fold runs before its tail
                                                 (2, 2300, 64, 8, True, True)])
def test_groupnorm(B, HW, C, G, silu, train):
    KC.case_groupnorm(DEV, B, HW, C, G, silu, train_params=train)


@pytest.mark.parametrize("what,B,HW,C,G,knobs,lo,deferred", KC.GN_INSTANTIATION_CASES, ids=[c[0] for c in KC.GN_INSTANTIATION_CASES])
def test_groupnorm_instantiations_no_other_case_reaches(what, B, HW, C, G, knobs, lo, deferred):
    """two column chunks per thread, the remainder under "gn_unroll", the 512-thread 8-row forward, the 16-row forward and 512-thread
    backward folding a deferred producer"""
    KC.case_groupnorm_instantiation(DEV, B, HW, C, G, knobs, lo, deferred)


@pytest.mark.parametrize("B,HW,Ca,Cb,G,silu", [(4, 4096, 320, 320, 32, True), (4, 4096, 640, 320, 32, True), (4, 1024, 640, 640, 32, True),
                                               (4, 1024, 1280, 640, 32, True), (4, 256, 1280, 1280, 32, True), (4, 64, 1280, 1280, 32, True),
                                               (1, 300, 64, 32, 8, False)])
def test_groupnorm_concat_in_place(B, HW, Ca, Cb, G, silu):
    """the up-path resnets' norm1 at the train shapes (512^2 bs 4): concatenation read in place == materialised, bit for bit"""
    KC.case_groupnorm_concat(DEV, B, HW, Ca, Cb, G, silu)


@pytest.mark.parametrize("B,HW,C,Kd,G,split,lora", [(4, 256, 1280, 2560, 32, 4, False), (4, 1024, 640, 640, 32, 2, True), (4, 64, 1280, 1280, 32, 6, True),
                                                    (4, 4096, 320, 320, 32, 2, False),   # 64x64 maps: two-launch plan, finished first
                                                    (2, 16, 128, 256, 8, 2, False), (4, 256, 1280, 1280, 32, 3, True), (2, 64, 64, 128, 8, 1, False)])
def test_deferred_split_k_finish_in_the_norm_kernels(B, HW, C, Kd, G, split, lora):
    KC.case_deferred_finish(DEV, B, HW, C, Kd, G, split, lora=lora)


@pytest.mark.parametrize("M,Kd,tile,lora,res", [(16384, 320, 55, True, True), (16384, 320, 55, False, False), (16384, 1280, 55, False, True),
                                                (32768, 320, 54, True, True), (16384, 320, 52, True, True), (1000, 320, 51, False, True)])
def test_gemm_fused_layernorm(M, Kd, tile, lora, res):
    """the level-0 projections (16384 x 320) with the LayerNorm that follows them written by the same launch"""
    KC.case_gemm_fused_layernorm(DEV, M, Kd, tile, lora=lora, residual=res)


@pytest.mark.parametrize("M,C", [(4096, 320), (1024, 640), (259, 1280)])
def test_layernorm(M, C):
    KC.case_layernorm(DEV, M, C)


@pytest.mark.parametrize("M,C", [(16384, 320), (4099, 640), (2049, 1280), (1024, 1280), (308, 768)])
def test_layernorm_rows_in_flight(M, C):
    KC.case_layernorm_rows(DEV, M, C)


def test_geglu():
    KC.case_geglu(DEV, 4096, 1280)


def test_geglu_past_the_grid_cap():
    KC.case_geglu(DEV, 4100, 2056)


@pytest.mark.parametrize("M,K,N,R,xr", [(8192, 320, 320, 4, 0), (8192, 320, 320, 8, 4096), (308, 768, 640, 8, 0), (512, 576, 320, 32, 0),
                                        (2113, 72, 520, 4, 0),       # 34 row slabs: the finish pass's eight-loads-in-flight loop, a second column block
                                        (8200, 72, 1032, 4, 0)])     # lora_up past its 4096-block cap
def test_lora(M, K, N, R, xr):
    KC.case_lora(DEV, M, K, N, R, x_rows=xr)


def test_lora_wgrad_jobs_of_different_sizes_in_one_launch():
    KC.case_lora_wgrad_multi(DEV)


@pytest.mark.parametrize("kw", [dict(Mc=16384, Cc=320, C_=320, rc=4, n=10), dict(Mc=4096, Cc=640, C_=640, rc=4, n=10),
                                dict(Mc=256, Cc=1280, C_=1280, rc=8, n=2, strided_grad=False)])
def test_control_terms_in_rank_space(kw):
    """reference models.py:214-218, 237-238 at the level shapes of the step: the rank-space kernels vs torch autograd of the formula"""
    print("RANK_CONTROL", kw, KC.case_rank_control(DEV, **kw))


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_lora_down_launch_modes(mode):
    """option "lora_down_mode": how an adapter down-projection is spread over waves (K-split everywhere / eight k-steps in flight):
    same T within fp32 summation-order noise at the level-0 size, stacked q|k|v rows with a second input on the first adapter"""
    for M, Kd in ((16384, 320), (1024, 1280), (200, 1288), (256, 2560)):
        KC.case_lora_down_mode(DEV, mode, M, Kd)


def test_elementwise():
    KC.case_elementwise(DEV)


def test_loss_and_optimizer():
    KC.case_loss_and_optimizer(DEV, n=100000)


@pytest.mark.parametrize("n", [78080, 1024 * 256 + 300])
def test_grad_norm_is_the_same_bits_on_every_launch(n):
    """the DreamBooth test's flat LoRA buffer (305 blocks) and one element count past the 1024-block cap of clora_grad_sumsq_f32"""
    KC.case_grad_sumsq_reproducible(DEV, n, graph=True)


def test_loss_and_optimizer_past_the_grid_caps():
    """mse caps its grid at 256 blocks, grad_sumsq at 1024, AdamW at 4096: 300 elements into the second trip of the widest"""
    KC.case_loss_and_optimizer(DEV, n=4096 * 256 + 300)


@pytest.mark.parametrize("M,N", [(1030, 130), (37, 8)])
def test_colsum(M, N):
    KC.case_colsum(DEV, M, N)


def test_elementwise_past_the_grid_cap():
    KC.case_elementwise_past_cap(DEV)


def test_copies_past_the_grid_cap():
    KC.case_copies_past_cap(DEV)


@pytest.mark.parametrize("B,H,W,C", [(2, 5, 7, 24), (1, 513, 1023, 16)])        # the second: 1022 vectors past the cap
def test_pool2x2_sum(B, H, W, C):
    KC.case_pool2x2_sum(DEV, B, H, W, C)


@pytest.mark.parametrize("rows,cols", [(4096, 4096), (1000, 72), (7, 8192)])
def test_softmax_rows(rows, cols):
    KC.case_softmax_rows(DEV, rows, cols)


def test_conv_padded_channels_pack_and_oihw_grad():
    KC.case_conv_padded_channels(DEV)


@pytest.mark.parametrize("kw", [dict(stride=2, pad=1), dict(asym=True, stride=2, pad=0), dict(ups=True)])
def test_conv_fast_path_variants(kw):
    """strided / asymmetric-pad / upsampled 3x3 gathers and their dgrads at Cin % 32 == 0 (generic gather path; the
    wave-uniform fast path is reserved for stride-1: a tabulated-offset generalisation measured no faster than generic)"""
    KC.case_conv(DEV, 2, 16, 16, 64, 96, **kw)
    KC.case_conv(DEV, 1, 32, 32, 320, 320, **kw)


@pytest.mark.parametrize("tile", [0, 1, 7, 8, 21, 31, 41, 53, 56])
def test_feed_forward_fused_geglu(tile):
    KC.case_feed_forward_fused(DEV, M=1000, C=320, tile_cfg=tile)
    KC.case_feed_forward_fused(DEV, M=300, C=1280, tile_cfg=tile)


@pytest.mark.parametrize("tile", [0, 1, 2, 3, 7, 8, 21, 22, 23, 26, 41, 43])
def test_conv_channel_chunk_major_k_order(tile):
    """clora_conv_t.kchunk = 64 (what ops.ConvPack uses for every UNet conv) at real widths, forward and dgrad, plus the
    strided / upsampled gathers"""
    KC.case_conv(DEV, 2, 32, 32, 320, 640, tile_cfg=tile, kchunk=64)
    KC.case_conv(DEV, 1, 16, 16, 1280, 1280, tile_cfg=tile, kchunk=64)
    for kw in (dict(stride=2, pad=1), dict(asym=True, stride=2, pad=0), dict(ups=True)):
        KC.case_conv(DEV, 1, 16, 16, 128, 64, tile_cfg=tile, kchunk=64, **kw)


@pytest.mark.parametrize("family", ["attention", "groupnorm", "layernorm", "lora_up", "lora_wgrad", "conv_patch", "conv_patch_splitk"])
def test_kernels_are_bit_stable_run_to_run(family):
    """Two identical launches must give identical bits at the level-0 shapes of the step (every kernel here is atomics-free by
    design): the guard that caught a sporadically wrong GEMM epilogue variant in round 3, extended to the other kernel families."""
    import math
    g = torch.Generator().manual_seed(71)
    f32 = torch.float32
    big = DEV == "cuda"                       # (the CPU harness in tests/test_kernels_emu.py drives the same body at small sizes)
    if family == "attention":
        B, H, N, D = (2, 8, 4096, 40) if big else (1, 2, 200, 40)
        qkv, dO = KC.rnd((B * N, 3 * H * D), DEV, g), KC.rnd((B * N, H * D), DEV, g)
        q, k, v = qkv[:, :H * D], qkv[:, H * D:2 * H * D], qkv[:, 2 * H * D:]

        def run():
            o, lse = K.attn_fwd(q, k, v, B, H, N, N, D, D ** -0.5)
            d = torch.empty_like(qkv)
            K.attn_bwd(q, k, v, o, dO, lse, B, H, N, N, D, D ** -0.5, d[:, :H * D], d[:, H * D:2 * H * D], d[:, 2 * H * D:])
            return o, lse, d
    elif family == "groupnorm":
        x, dy, dres = (KC.rnd((4, 4096, 320) if big else (2, 60, 320), DEV, g) for _ in range(3))
        gamma, beta = KC.rnd((320,), DEV, g, dtype=f32), KC.rnd((320,), DEV, g, dtype=f32)

        def run():
            y, st = K.groupnorm_fwd(x, gamma, beta, 32, 1e-5, True)
            dx, _, _ = K.groupnorm_bwd(x, dy, gamma, beta, st, 32, True, dres=dres)
            return y, st, dx
    elif family == "layernorm":
        x, dy, dres = (KC.rnd((16384 if big else 70, 320), DEV, g) for _ in range(3))
        gamma, beta = KC.rnd((320,), DEV, g, dtype=f32), KC.rnd((320,), DEV, g, dtype=f32)

        def run():
            return K.layernorm_fwd(x, gamma, beta, 1e-5), K.layernorm_bwd(x, dy, gamma, 1e-5, dres=dres)
    elif family == "lora_up":
        M, N = (16384 if big else 200), 320
        base, T, U = KC.rnd((M, N), DEV, g), KC.rnd((M, 4), DEV, g, dtype=f32), KC.rnd((N, 4), DEV, g, dtype=f32)

        def run():
            return (K.lora_up(base, T, 0, U, M, N, 0.7),)
    elif family == "lora_wgrad":
        M, N = (16384 if big else 300), 320
        A, T = KC.rnd((M, N), DEV, g), KC.rnd((M, 4), DEV, g, dtype=f32)

        def run():
            G = torch.zeros((N, 4), dtype=f32, device=DEV)
            K.lora_wgrad(A, T, 0, G, 4, 1, M, N, 4, scale=0.5)
            return (G,)
    else:
        from controllora_amd.ops import conv_k_order
        Bn, Hh, Ci, Co = (4, 64, 320, 320) if big else (1, 16, 128, 160)
        M = Bn * Hh * Hh
        x = KC.rnd((M, Ci), DEV, g)
        w = conv_k_order(KC.rnd((Co, 9, Ci), DEV, g, 1 / math.sqrt(9 * Ci)), 64)
        res = KC.rnd((M, Co), DEV, g)
        cd, _, _ = K.conv_fwd_desc(Hh, Hh, Ci, 3, 1, 1, kchunk=64)
        sk = 2 if family == "conv_patch_splitk" else 1

        def run():
            return (K.gemm(x, w, M, Co, 9 * Ci, conv=cd, residual=res, tile_cfg=76, split_k=sk, _tuned=False),)
    a, b = run(), run()
    torch.cuda.synchronize() if DEV == "cuda" else None
    for u, v_ in zip(a, b):
        assert torch.equal(u, v_), f"{family}: two identical launches differ in {int((u != v_).sum())} elements"
        assert bool(torch.isfinite(u.float()).all())


def test_every_plain_entry_of_the_tuned_table_is_exact_and_bit_stable():
    """The autotuned launch table (controllora_amd/gemm_tuning_gfx950.json) entry by entry, for the plain (non-conv) signatures of the
    train step and the batch-32 inference forward: each (shape, tile_cfg, split_k) with a bias + rank-4 adapter + residual epilogue
    against an fp32 matmul -- rel-L2, no outlier element, and two identical launches bit-identical (the guard that caught tile_cfg 42)."""
    import json
    import math
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(K.__file__)), "gemm_tuning_gfx950.json")
    table = json.load(open(path))["table"]
    g = torch.Generator().manual_seed(81)
    done = 0
    for key, (tile, sk) in sorted(table.items()):
        if ":" in key:
            continue
        M, N, Kd = (int(v) for v in key.split("x"))
        if M * N * Kd > 6e10 or M * N > 3.4e7 or N % 16 or M < 16:        # keep the whole sweep to seconds; the big ones share their kernels
            continue
        A, B = KC.rnd((M, Kd), DEV, g), KC.rnd((N, Kd), DEV, g, 1 / math.sqrt(Kd))
        bias, res = KC.rnd((N,), DEV, g, dtype=torch.float32), KC.rnd((M, N), DEV, g)
        T, U = KC.rnd((M, 4), DEV, g, dtype=torch.float32), KC.rnd((N, 4), DEV, g, 0.3, dtype=torch.float32)
        ref = ((A.float() @ B.float().T) + bias + T @ U.T).half().float() + res.float()
        kw = dict(bias=bias, residual=res, lora_t=T, lora_u=U, lora_seg=N, tile_cfg=tile, split_k=sk, _tuned=False)
        out = K.gemm(A, B, M, N, Kd, **kw)
        again = K.gemm(A, B, M, N, Kd, **kw)
        e = float((out.float() - ref).norm() / ref.norm())
        assert e < 8e-4, (key, tile, sk, e)
        assert torch.equal(out, again), (key, tile, sk, "two identical launches differ")
        lim = 6e-3 * max(1.0, float(ref.abs().max()))
        worst = float((out.float() - ref).abs().max())
        assert worst < lim, (key, tile, sk, worst, lim)
        done += 1
    assert done >= 60, done


@pytest.mark.parametrize("waves", [4, 8, 16])
@pytest.mark.parametrize("B,H,Nq,Nk,D", [(2, 8, 4096, 4096, 40), (1, 2, 600, 300, 40), (2, 1, 513, 64, 40), (1, 8, 1024, 1100, 64)])
def test_attention_forward_block_widths(waves, B, H, Nq, Nk, D):
    """clora_set_option("attn_fwd_waves"): 4 / 8 / 16 waves = 128 / 256 / 512 queries per forward block (the 16-wave block halves the
    K/V tile stream per flop once more: the batch-32 sampler's level-0 self-attention); same results, ragged query counts included"""
    from controllora_amd import kernels as K_
    K_.set_option("attn_fwd_waves", waves)
    try:
        KC.case_attention(DEV, B, H, Nq, Nk, D)
    finally:
        K_.set_option("attn_fwd_waves", 0)


def test_groupnorm_team_exchange_under_graph_replay_and_changing_geometry():
    """The team kernels' in-launch exchange (include/clora.h clora_groupnorm_*_team) with everything that could expose a stale word:
    launches of four geometries (8 / 16 / 32 units, 32 / 16 / 8 / 64 members) interleaved so that granule slots are re-used by units
    whose epochs differ, 40 launch pairs captured in ONE hipGraph and replayed (frozen arguments: the epoch must come from the state),
    consumers that have just read the same lines (L1-warm), a GEMM between the launches so that workgroups start unevenly.  Every
    replay must give the bits of the first eager pass, which in turn agree with the two-launch scheme; no exchange may give up."""
    g = torch.Generator().manual_seed(5)
    f32 = torch.float32
    shapes = [(4, 4096, 320), (4, 1024, 640), (8, 1024, 320), (2, 4096, 320), (4, 1024, 1280)]
    data = []
    for B, HW, C in shapes:
        x, dy = KC.rnd((B, HW, C), DEV, g), KC.rnd((B, HW, C), DEV, g)
        gamma, beta = 1 + 0.2 * KC.rnd((C,), DEV, g, dtype=f32), 0.2 * KC.rnd((C,), DEV, g, dtype=f32)
        data.append((x, dy, gamma, beta))
    A, W = KC.rnd((4096, 640), DEV, g), KC.rnd((640, 640), DEV, g)

    def one_pass():
        outs = []
        for rep in range(4):
            for x, dy, gamma, beta in data:
                y, st = K.groupnorm_fwd(x, gamma, beta, 32, 1e-5, True)
                K.gemm(A, W, 4096, 640, 640)
                dx, _, _ = K.groupnorm_bwd(x, dy, gamma, beta, st, 32, True)
                if rep == 3:
                    outs += [y, st, dx]
        return outs

    K.set_option("gn_team", 0)
    try:
        ref = one_pass()
    finally:
        K.set_option("gn_team", int(os.environ.get("CLORA_GN_TEAM", "2")))
    first = one_pass()
    for a, b in zip(first, ref):
        assert KC.rel(a, b) < 3e-4
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = one_pass()
    for _ in range(5):
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(captured, first):
            assert torch.equal(a, b)
    assert K.gn_team_errors(DEV) == 0


@pytest.mark.parametrize("B,HW,C,G,units,units_bwd", KC.TEAM_NARROW_SHAPES)
def test_groupnorm_team_narrow_slabs_and_large_teams(B, HW, C, G, units, units_bwd):
    """the VAE's norms on the team kernels (CS < 160, 64 / 128 / 256 members, ragged members), each with its plan asserted"""
    KC.case_groupnorm_team_narrow(DEV, B, HW, C, G, HW != 1030, units=units, units_bwd=units_bwd)


def test_groupnorm_team_narrow_away_from_zero_mean():
    """mean 10 std at the 64- and 128-member geometries: every member of a unit subtracts the same pivot"""
    for B in (4, 2):
        KC.case_groupnorm_team_narrow(DEV, B, 4096, 16, 8, False, units=B, offset=10.0)


@pytest.mark.parametrize("level,B,HW,C,G,units,units_bwd,backward", KC.TEAM_LEVEL_SHAPES)
def test_groupnorm_team_option_levels(level, B, HW, C, G, units, units_bwd, backward):
    """"gn_team" 3 / 4 put the 16x16 / 8x8 maps on the team kernels; at the default the same call must not take them"""
    KC.case_groupnorm_team_narrow(DEV, B, HW, C, G, True, level=level, units=units, units_bwd=units_bwd, backward=backward)


def test_groupnorm_team_alternating_64_and_128_members():
    KC.case_groupnorm_team_alternating(DEV, graph=True)


@pytest.mark.parametrize("M,N,K_,split,tile,lora", [(16384, 320, 320, 1, 0, False), (16384, 320, 320, 1, 55, True), (1024, 1280, 1280, 3, 0, False),
                                                   (4096, 640, 2560, 1, 0, False), (300, 96, 64, 1, 1, False)])
def test_gemm_compensated_trunk(M, N, K_, split, tile, lora):
    KC.case_gemm_trunk_lo(DEV, M, N, K_, split_k=split, tile_cfg=tile, lora=lora)


# ---- every attention instantiation, both backward widths, the causal entry point, the option table (fp64 references)
@pytest.mark.parametrize("D", list(range(8, 161, 8)))
def test_attention_full_every_head_size(D):
    """every <DP, DT, ONES> instantiation the C ABI dispatches to, each its own code object with its own register and LDS budget:
    ragged query blocks and KV tiles, output, LSE and gradients against fp64"""
    KC.case_attention_full(DEV, 2, 4, 1000, 300, D, strided=(D // 8) % 3 == 0)


SD15_SITES = [(2, 8, 4096, 4096, 40), (2, 8, 1024, 1024, 80), (2, 8, 256, 256, 160)]      # self-attention, SURVEY.md Appendix B


@pytest.mark.parametrize("q_scale", [1.0, 6.0])
@pytest.mark.parametrize("B,H,Nq,Nk,D", SD15_SITES)
def test_attention_full_sd15_sites(B, H, Nq, Nk, D, q_scale):
    """the three self-attention sites with the gradients as column blocks of one buffer (the fused q | k | v projection's dgrad input),
    ordinary and peaked (q x 6) softmax"""
    KC.case_attention_full(DEV, B, H, Nq, Nk, D, q_scale=q_scale, strided=True)


@pytest.mark.parametrize("B,H,Nq,Nk,D", [(2, 2, 1, 1, 40), (1, 2, 5, 8, 64), (2, 3, 129, 65, 104), (2, 3, 129, 65, 24)])
def test_attention_full_edge_shapes(B, H, Nq, Nk, D):
    KC.case_attention_full(DEV, B, H, Nq, Nk, D)


@pytest.mark.parametrize("B,H,Nq,Nk,D", [(3, 5, 1000, 1000, D) for D in range(8, 65, 8)] + [(2, 8, 1100, 300, 32), (2, 8, 4096, 77, 40)])
def test_attention_block_widths_against_reference(B, H, Nq, Nk, D):
    """"attn_bwd_waves" 4 | 8 x "attn_fwd_waves" 4 | 6 | 8 | 16 with partial last query and key blocks at every width (4096 x 77: the
    query-split dK/dV path): reference parity and the same bits as the 4-wave kernels"""
    KC.case_attention_widths(DEV, B, H, Nq, Nk, D, strided=D in (40, 64))


@pytest.mark.parametrize("D", list(range(8, 65, 8)))
@pytest.mark.parametrize("N", [1, 8, 63, 64, 65, 77, 128, 129, 300, 1000])
def test_attention_causal(N, D):
    KC.case_attention_causal(DEV, 2, 3, N, D, strided=N != 63)


@pytest.mark.parametrize("B", [4, 32])
def test_attention_causal_clip_l_shape(B):
    KC.case_attention_causal(DEV, B, 12, 77, 64)


def test_attention_causal_rejects_wide_heads():
    KC.case_attention_causal_rejects(DEV, 72)


# ---- eight distinct leading dimensions; the query-split dK/dV path: the shapes of tests/test_kernels_emu.py (tests/test_attention_mutants_emu.py
# says what each is for), a few milliseconds each on the device
@pytest.mark.parametrize("B,H,Nq,Nk,D", [(2, 2, 70, 150, 40), (2, 2, 70, 150, 64), (2, 1, 70, 150, 80), (2, 1, 40, 70, 160),
                                         (2, 2, 513, 77, 40), (1, 2, 513, 77, 128)])
def test_attention_distinct_strides(B, H, Nq, Nk, D):
    KC.case_attention_strides(DEV, B, H, Nq, Nk, D, waves=(0, 8) if D <= 64 and Nq < 512 else (0,))


def test_attention_causal_distinct_strides():
    KC.case_attention_strides(DEV, 2, 2, 77, 77, 64, causal=True)


@pytest.mark.parametrize("D", [8, 32, 40, 64, 80, 96, 128, 160])
def test_attention_split_every_instantiation(D):
    KC.case_attention_split(DEV, 2, 2, 513, 77, D, splits=3)


@pytest.mark.parametrize("B,H,Nq,Nk,D,splits", [(1, 1, 1100, 77, 40, 6), (1, 1, 1300, 77, 16, 7)])
def test_attention_split_fold_tail(B, H, Nq, Nk, D, splits):
    KC.case_attention_split(DEV, B, H, Nq, Nk, D, splits=splits, strided=False, tail=True)


def test_attention_split_five_ways():
    KC.case_attention_split(DEV, 1, 2, 640, 77, 40, splits=5)


def test_attention_split_fold_second_grid_stride_trip():
    KC.case_attention_split(DEV, 1, 14, 512, 1024, 160, splits=4)


def test_attention_workspace_budget():
    KC.case_attention_workspace(DEV, 2, 2, 1100, 77, 40)


OPTION_VALUES = [("epi_hoist", 0), ("epi_two_phase", 0), ("gn_unroll", 1), ("gn_blocks", 64), ("gn_blocks", 4096),
                 ("strip_blocks", 64), ("strip_blocks", 16384), ("wgrad_patch", 128)]


@pytest.mark.parametrize("name,value", OPTION_VALUES)
def test_option_table(name, value):
    """include/clora.h, the table above clora_set_option: reference parity at the default and at the other value, and the same bits
    across the two wherever the header promises them"""
    KC.case_option_invariance(DEV, name, value)


@pytest.mark.parametrize("offset", [0, 10, 30, 100])
@pytest.mark.parametrize("B,HW,C,G", [(4, 4096, 320, 32), (4, 256, 1280, 32), (4, 1024, 640, 32), (3, 1000, 640, 32), (2, 300, 64, 8)])
def test_groupnorm_away_from_zero_mean(B, HW, C, G, offset):
    """|mean| / std up to 100 under every plan: team (64x64, 32x32 maps), one block per slab (16x16), two launches (batch 3)"""
    KC.case_groupnorm_offset(DEV, B, HW, C, G, offset, silu=HW == 300)


def test_groupnorm_offset_300_is_reported_not_asserted():
    """fp16 carries about two bits of a unit-variance signal at 300: the measured error is printed (include/clora.h, GroupNorm entry)"""
    for shape in ((4, 4096, 320, 32), (4, 256, 1280, 32)):
        print("GN_OFFSET_300", shape, KC.case_groupnorm_offset(DEV, *shape, 300, check=False))
