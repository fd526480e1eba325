"""Every refusal of every GEMM entry (csrc/gemm_run.inc) over the emulation library: one row per entry and cause, with the return code
the entry gave before its host side became one file and gives now (tools/gemm_emu_compare.py makes the calls and compared the two
builds).  Nothing is launched by any of them."""
import pytest

from tests.emu_build import load_emu
from tools.gemm_emu_compare import refusals

E_ARG, E_ALIGN = -1, -3
TABLE = [
    ("linear_f32 null A", E_ARG),
    ("linear_f32 M=0", E_ARG),
    ("linear_f32 ldw < K", E_ARG),
    ("linear_f32 ldw % 4", E_ALIGN),
    ("linear_f32 misaligned W", E_ALIGN),
    ("linear_f32 group 0", E_ARG),
    ("linear_f32 group 7 (80 % group)", E_ARG),
    ("linear_f32 group 16 (N % group)", E_ARG),
    ("linear_f32 resid with sigmoid", E_ARG),
    ("linear_f32 unknown mode", E_ARG),
    ("linear_pack_bf16x3 null planes", E_ARG),
    ("linear_pack_bf16x3 ld_in < K", E_ARG),
    ("linear_pack_bf16x3 ld_out % 32", E_ARG),
    ("linear_bf16x3 null planes", E_ARG),
    ("linear_bf16x3 ldw < K", E_ARG),
    ("linear_bf16x3 ldw % 32", E_ALIGN),
    ("linear_bf16x3 misaligned planes", E_ALIGN),
    ("linear_bf16x3 group 0", E_ARG),
    ("linear_bf16x3 group 3 (160 % group)", E_ARG),
    ("linear_bf16x3 group 16 (N % group)", E_ARG),
    ("linear_bf16x3 resid without L2NORM", E_ARG),
    ("linear_bf16x3 RELU", E_ARG),
    ("x3_image null img", E_ARG),
    ("x3_image rows=0", E_ARG),
    ("x3_image misaligned img", E_ALIGN),
    ("x3_image_t null src", E_ARG),
    ("x3_image_t ld < M", E_ARG),
    ("x3_image_t misaligned img", E_ALIGN),
    ("x3_image_both null img_t", E_ARG),
    ("x3_image_both ld < M", E_ARG),
    ("x3_image_both misaligned img_rows", E_ALIGN),
    ("x3_image_both_colsum null colsum", E_ARG),
    ("x3_image_both_colsum misaligned img_t", E_ALIGN),
    ("linear_x3p null a_img", E_ARG),
    ("linear_x3p misaligned a_img", E_ALIGN),
    ("linear_x3p KB overflow", E_ARG),
    ("linear_x3p pairs", E_ARG),
    ("linear_x3p pairs, bf16", E_ARG),
    ("linear_x3p group 0", E_ARG),
    ("linear_x3p group 10 (group % 4)", E_ARG),
    ("linear_x3p group 8 (80 / group > 4)", E_ARG),
    ("linear_x3p group 16 (80 % group)", E_ARG),
    ("linear_x3p group 80 (N % group)", E_ARG),
    ("linear_x3p RELU", E_ARG),
    ("linear_x3p null AND misaligned", E_ARG),
    ("linear_x3p_norms null inv_norm", E_ARG),
    ("linear_x3p_norms group 2", E_ARG),
    ("linear_x3p_norms group 16", E_ARG),
    ("linear_x3p_norms KB overflow", E_ARG),
    ("linear_x3p_resid group 0", E_ARG),
    ("linear_x3p_resid group 3", E_ARG),
    ("linear_x3p_resid group 8", E_ARG),
    ("linear_x3p_resid group 16 (N % group)", E_ARG),
    ("linear_x3p_resid resid_mod 0", E_ARG),
    ("linear_x3p_resid misaligned w_img", E_ALIGN),
    ("linear_x3p_resid KB overflow", E_ARG),
    ("linear_x3p_resid KB overflow, no residual", E_ARG),
    ("linear_x3p_pair null C2", E_ARG),
    ("linear_x3p_pair group 2", E_ARG),
    ("linear_x3p_pair group 8", E_ARG),
    ("linear_x3p_pair n_split 0", E_ARG),
    ("linear_x3p_pair n_split = N", E_ARG),
    ("linear_x3p_pair n_split % group", E_ARG),
    ("linear_x3p_pair misaligned a_img", E_ALIGN),
    ("linear_x3p_pair KB overflow", E_ARG),
    ("linear_x3p_pair bad group AND misaligned", E_ARG),
    ("linear_x3p_compact null dest", E_ARG),
    ("linear_x3p_compact F=0", E_ARG),
    ("linear_x3p_compact group 2", E_ARG),
    ("linear_x3p_compact N != F * group", E_ARG),
    ("linear_x3p_compact misaligned comp", E_ALIGN),
    ("linear_x3p_compact comp_bs % 4", E_ALIGN),
    ("linear_x3p_compact KB overflow", E_ARG),
    ("linear_x3p_batched ldc < N", E_ARG),
    ("linear_x3p_batched batch 0", E_ARG),
    ("linear_x3p_batched batch 65536", E_ARG),
    ("linear_x3p_batched a_bs % 8", E_ALIGN),
    ("linear_x3p_batched misaligned a_img", E_ALIGN),
    ("linear_x3p_batched KB overflow", E_ARG),
    ("linear_x3p_batched_split null C2", E_ARG),
    ("linear_x3p_batched_split n_split 0", E_ARG),
    ("linear_x3p_batched_split n_split = N", E_ARG),
    ("linear_x3p_batched_split w_bs % 8", E_ALIGN),
    ("linear_x3p_batched_split batch 65536", E_ARG),
    ("linear_x3p_batched_split_alt null C2", E_ARG),
    ("linear_x3p_batched_split_alt n_split_odd 0", E_ARG),
    ("linear_x3p_batched_split_alt n_split_odd < 0", E_ARG),
    ("linear_x3p_batched_split_alt n_split_odd = N", E_ARG),
    ("linear_x3p_batched_split_alt n_split = N", E_ARG),
    ("lstm_wgrad_images null zero16", E_ARG),
    ("lstm_wgrad_images NP % 32", E_ARG),
    ("lstm_wgrad_images Hp % 8", E_ARG),
    ("lstm_wgrad_images image overflow", E_ARG),
    ("lstm_wgrad_images misaligned dp_img", E_ALIGN),
    ("linear_x3t ldc < N", E_ARG),
    ("linear_x3t K=0", E_ARG),
    ("linear_x3t image overflow", E_ARG),
    ("linear_x3t misaligned zero16", E_ALIGN),
]


@pytest.fixture(scope="module")
def codes():
    return dict(refusals(load_emu()))


def test_the_table_names_every_refusal_call(codes):
    assert sorted(codes) == sorted(name for name, _ in TABLE)


@pytest.mark.parametrize("name,code", TABLE)
def test_gemm_entry_refuses(codes, name, code):
    assert codes[name] == code
