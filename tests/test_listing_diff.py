"""tools/listing_diff.py's normalisation, pinned on two tiny synthetic listings (host only): a renumbered local label and a kernel
renamed into the mapping templates compare equal; a swapped operand, and a kernel that one side lacks, do not."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import listing_diff as LD  # noqa: E402

OLD_SYMBOL = "_ZN2mc12_GLOBAL__N_121mandel_perturb_kernelILi8EEEvNS0_11PerturbArgsE"
NEW_SYMBOL = "_ZN2mc12_GLOBAL__N_117mandelbrot_kernelINS0_12StatePerturbELi8EEEvNT_4ArgsE"


def listing(symbol, index, add="v_add3_u32 v2, v0, v1, v3", cuid="0123"):
    """One kernel as `hipcc -S` writes it: directives, comments, local labels numbered by the kernel's position in its file."""
    return f"""\t.text
\t.globl\t{symbol}
\t.type\t{symbol},@function
{symbol}:                               ; @{symbol}
; %bb.0:
\ts_load_dwordx2 s[2:3], s[0:1], 0x0
.LBB{index}_1:                          ; =>This Inner Loop Header: Depth=1
\t{add}           ; a trailing comment
\ts_cbranch_scc1 .LBB{index}_1
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel {symbol}
\t\t.amdhsa_next_free_vgpr 4
\t.end_amdhsa_kernel
\t.text
.Lfunc_end{index}:
\t.size\t{symbol}, .Lfunc_end{index}-{symbol}
\t.type\t__hip_cuid_{cuid},@object
__hip_cuid_{cuid}:
"""


def test_kernel_names_come_from_the_symbol():
    assert LD.kernel_name(OLD_SYMBOL) == ("mandel_perturb_kernel", 8)
    assert LD.kernel_name(NEW_SYMBOL) == ("mandelbrot_kernel", "StatePerturb", 8)
    assert LD.renamed(LD.kernel_name(OLD_SYMBOL)) == LD.kernel_name(NEW_SYMBOL)
    assert LD.kernel_name("_ZN2mc12_GLOBAL__N_117mandelbrot_kernelINS0_8StateF32ILb0EEELi8EEEvNS0_10MandelArgsE") == \
        LD.kernel_name("_ZN2mc12_GLOBAL__N_117mandelbrot_kernelINS0_8StateF32ILb0EEELi8EEEvNT_4ArgsE") == \
        ("mandelbrot_kernel", "StateF32", 0, 8)
    assert LD.kernel_name("plain_c_kernel") == ("plain_c_kernel",)


def test_a_bla_template_that_names_its_policy_is_not_renamed_again():
    """The BLA units' tile kernel had the name its template has now.  The old kernels go to their policies; a first directory that already
    holds the template compares with itself."""
    old_tile = "_ZN2mc12_GLOBAL__N_125mandel_perturb_bla_kernelENS_14PerturbBlaArgsE"
    old_list = "_ZN2mc12_GLOBAL__N_130mandel_perturb_bla_list_kernelENS_14PerturbBlaArgsENS_10SampleListE"
    new_tile = "_ZN2mc12_GLOBAL__N_125mandel_perturb_bla_kernelINS0_7MapTileEJEEEvNS_14PerturbBlaArgsEDpT0_"
    new_list = "_ZN2mc12_GLOBAL__N_125mandel_perturb_bla_kernelINS0_7MapListEJNS_10SampleListEEEEvNS_14PerturbBlaArgsEDpT0_"
    assert LD.renamed(LD.kernel_name(old_tile)) == LD.kernel_name(new_tile) == ("mandel_perturb_bla_kernel", "MapTile")
    assert LD.renamed(LD.kernel_name(old_list)) == LD.kernel_name(new_list) == ("mandel_perturb_bla_kernel", "MapList")
    for symbol in (new_tile, new_list):
        assert LD.renamed(LD.kernel_name(symbol)) == LD.kernel_name(symbol)
    both = listing(new_tile, 0) + listing(new_list, 1)
    lines, bad = LD.compare(both, both)
    assert bad == 0 and lines == ["mandel_perturb_bla_kernel<MapList>: identical", "mandel_perturb_bla_kernel<MapTile>: identical"]


def test_label_renumbering_and_rename_compare_equal():
    lines, bad = LD.compare(listing(OLD_SYMBOL, 0, cuid="aaaa"), listing(NEW_SYMBOL, 3, cuid="bbbb"))
    assert bad == 0 and lines == ["mandelbrot_kernel<StatePerturb, 8>: identical"]


def test_swapped_operand_differs():
    lines, bad = LD.compare(listing(OLD_SYMBOL, 0), listing(NEW_SYMBOL, 0, add="v_add3_u32 v2, v1, v0, v3"))
    assert bad == 1 and "DIFFERS at instruction 2" in lines[0]
    assert "    - v_add3_u32 v2, v0, v1, v3" in lines and "    + v_add3_u32 v2, v1, v0, v3" in lines


def test_kernel_on_one_side_only_is_a_difference():
    both = listing(OLD_SYMBOL, 0) + listing("_ZN2mc12_GLOBAL__N_126mandel_perturb_list_kernelILi8EEEvNS0_11PerturbArgsENS_10SampleListE", 1)
    lines, bad = LD.compare(both, listing(NEW_SYMBOL, 0))
    assert bad == 1 and "mandelbrot_list_kernel<StatePerturb, 8>: only in the first directory" in lines
    lines, bad = LD.compare(listing(NEW_SYMBOL, 0), both.replace(OLD_SYMBOL, NEW_SYMBOL))
    assert bad == 1 and "mandel_perturb_list_kernel<8>: only in the second directory" in lines


def test_resource_figures_are_compared_where_both_sides_have_them():
    def remarks(symbol, vgprs):
        tail = "[-Rpass-analysis=kernel-resource-usage]"
        return f"x.hip:1:1: remark: Function Name: {symbol} {tail}\nx.hip:1:1: remark:     VGPRs: {vgprs} {tail}\n"
    old, new = listing(OLD_SYMBOL, 0), listing(NEW_SYMBOL, 0)
    assert LD.compare(old, new, remarks(OLD_SYMBOL, 64), remarks(NEW_SYMBOL, 64))[1] == 0
    lines, bad = LD.compare(old, new, remarks(OLD_SYMBOL, 64), remarks(NEW_SYMBOL, 66))
    assert bad == 1 and "RESOURCES DIFFER: VGPRs 64 -> 66" in lines[0]
