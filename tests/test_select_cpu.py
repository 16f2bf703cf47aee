"""K5 / K9 kernel selection on the CPU: s2m2_amd/csrc/conv_select.h and chain_select.h are plain C++ (no HIP), so a small host program can print
the choice for a list of layers.  The list is every distinct layer the S model's forward sends to s2m2_conv2d and s2m2_mlp_chain at 1216 x 1024
(fp16; read off the binding during one forward), the 192-channel layers of the M model, pool2 / DUALMIX / pre-LayerNorm / shuffle2 layers, the
XCD grouping of K9, and forced tiles a layer cannot take.  EXPECTED was tabulated from the dispatchers as they were before selection became a
function of its own (their text compiled with the launchers stubbed to print their template arguments): a change of a line below is a change of
which kernel a layer runs on.

Choice format -- conv: family and the launcher's template parameters (igemm BM BN WGM PPR NPF NWAVES MODE / igemm2 BM BN KP NS /
halo BN NWAVES WGM DW / frag BN CH PH PW AUX / pw BN) or E:<error message>; chain: form, rows per tile, waves, weight tiles in flight, XCD tiles."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXPECTED = """
conv N=2 H=512 W=608 Cin=64 Cout=128 KH=3 KW=3 stride=1 epi=0 korder=0 pool2=0 ln=0 shuffle2=0 tile=0 fp16=1 -> halo 128 8 2 2
conv N=2 H=512 W=608 Cin=128 Cout=128 KH=3 KW=3 stride=1 epi=0 korder=2 pool2=0 ln=0 shuffle2=0 tile=0 fp16=1 -> frag 128 128 4 32 0
conv N=2 H=512 W=608 Cin=128 Cout=128 KH=3 KW=3 stride=1 epi=1 korder=2 pool2=0 ln=0 shuffle2=0 tile=0 fp16=1 -> frag 128 128 4 40 1
conv N=2 H=512 W=608 Cin=128 Cout=128 KH=3 KW=3 stride=2 epi=0 korder=0 pool2=0 ln=0 shuffle2=0 tile=0 fp16=1 -> igemm 128 128 2 4 1 8 0
conv N=2 H=256 W=304 Cin=128 Cout=128 KH=3 KW=3 stride=1 epi=0 korder=2 pool2=0 ln=0 shuffle2=0 tile=0 fp16=1 -> frag 128 128 4 40 0
conv N=2 H=256 W=304 Cin=128 Cout=128 KH=3 KW=3 stride=1 epi=1 korder=2 pool2=0 ln=0 shuffle2=0 tile=0 fp16=1 -> frag 128 128 4 40 1
conv N=2 H=64 W=76 Cin=256 Cout=256 KH=3 KW=3 stride=1 epi=0 korder=2 pool2=0 ln=0 shuffle2=0 tile=0 fp16=1 -> frag 128 128 2 32 0
conv N=2 H=64 W=76 Cin=256 Cout=256 KH=3 KW=3 stride=1 epi=1 korder=2 pool2=0 ln=0 shuffle2=0 tile=0 fp16=1 -> frag 128 128 2 32 1
conv N=1 H=1 W=19456 Cin=32 Cout=32 KH=1 KW=1 stride=1 epi=1 korder=0 pool2=0 ln=0 shuffle2=0 tile=0 fp16=1 -> igemm 128 32 4 8 1 4 0
conv N=1 H=256 W=304 Cin=136 Cout=128 KH=3 KW=3 stride=1 epi=0 korder=0 pool2=0 ln=0 shuffle2=0 tile=0 fp16=1 -> halo 128 8 2 2
conv N=1 H=256 W=304 Cin=128 Cout=128 KH=3 KW=3 stride=1 epi=0 korder=2 pool2=0 ln=0 shuffle2=0 tile=0 fp16=1 -> frag 128 128 4 40 0
conv N=1 H=256 W=304 Cin=128 Cout=128 KH=3 KW=3 stride=1 epi=1 korder=2 pool2=0 ln=0 shuffle2=0 tile=0 fp16=1 -> frag 128 128 4 40 1
conv N=1 H=256 W=304 Cin=256 Cout=384 KH=3 KW=3 stride=1 epi=0 korder=2 pool2=0 ln=0 shuffle2=0 tile=0 fp16=1 -> frag 128 128 4 40 0
conv N=1 H=256 W=304 Cin=384 Cout=128 KH=1 KW=1 stride=1 epi=5 korder=0 pool2=0 ln=0 shuffle2=0 tile=0 fp16=1 -> igemm 64 64 2 8 1 4 2
conv N=1 H=256 W=304 Cin=256 Cout=128 KH=3 KW=3 stride=1 epi=0 korder=2 pool2=0 ln=0 shuffle2=0 tile=0 fp16=1 -> frag 128 128 4 40 0
conv N=1 H=64 W=76 Cin=256 Cout=256 KH=3 KW=3 stride=1 epi=0 korder=2 pool2=0 ln=0 shuffle2=0 tile=0 fp16=1 -> frag 128 128 2 32 0
conv N=1 H=64 W=76 Cin=256 Cout=256 KH=3 KW=3 stride=1 epi=1 korder=2 pool2=0 ln=0 shuffle2=0 tile=0 fp16=1 -> frag 128 128 2 32 1
conv N=1 H=256 W=304 Cin=256 Cout=256 KH=3 KW=1 stride=1 epi=2 korder=2 pool2=0 ln=0 shuffle2=0 tile=0 fp16=1 -> frag 128 128 4 40 1
conv N=1 H=256 W=304 Cin=256 Cout=128 KH=3 KW=1 stride=1 epi=3 korder=0 pool2=0 ln=0 shuffle2=0 tile=0 fp16=1 -> halo 128 8 2 2
conv N=1 H=256 W=304 Cin=256 Cout=256 KH=1 KW=3 stride=1 epi=2 korder=2 pool2=0 ln=0 shuffle2=0 tile=0 fp16=1 -> frag 128 128 4 40 1
conv N=1 H=256 W=304 Cin=256 Cout=128 KH=1 KW=3 stride=1 epi=3 korder=0 pool2=0 ln=0 shuffle2=0 tile=0 fp16=1 -> halo 128 8 2 2
conv N=1 H=256 W=304 Cin=128 Cout=256 KH=3 KW=3 stride=1 epi=0 korder=2 pool2=0 ln=0 shuffle2=0 tile=0 fp16=1 -> frag 128 128 4 40 0
conv N=1 H=512 W=608 Cin=128 Cout=64 KH=3 KW=3 stride=1 epi=0 korder=0 pool2=0 ln=0 shuffle2=0 tile=0 fp16=1 -> halo 64 4 2 1
conv N=1 H=512 W=608 Cin=128 Cout=128 KH=3 KW=3 stride=1 epi=0 korder=2 pool2=0 ln=0 shuffle2=0 tile=0 fp16=1 -> frag 128 128 4 32 0
conv N=2 H=256 W=304 Cin=192 Cout=192 KH=3 KW=3 stride=1 epi=0 korder=2 pool2=0 ln=0 shuffle2=0 tile=0 fp16=1 -> frag 192 192 4 32 0
conv N=2 H=256 W=304 Cin=192 Cout=192 KH=3 KW=3 stride=1 epi=1 korder=2 pool2=0 ln=0 shuffle2=0 tile=0 fp16=1 -> frag 192 192 4 40 1
conv N=2 H=64 W=76 Cin=192 Cout=192 KH=3 KW=3 stride=1 epi=0 korder=2 pool2=0 ln=0 shuffle2=0 tile=0 fp16=1 -> frag 192 192 2 32 0
conv N=1 H=512 W=608 Cin=192 Cout=192 KH=3 KW=3 stride=1 epi=0 korder=2 pool2=0 ln=0 shuffle2=0 tile=0 fp16=1 -> frag 192 192 4 32 0
conv N=2 H=64 W=76 Cin=384 Cout=384 KH=3 KW=3 stride=1 epi=1 korder=2 pool2=0 ln=0 shuffle2=0 tile=0 fp16=1 -> frag 128 128 4 40 1
conv N=2 H=128 W=152 Cin=128 Cout=256 KH=1 KW=1 stride=1 epi=0 korder=0 pool2=1 ln=0 shuffle2=0 tile=0 fp16=1 -> igemm 64 64 2 4 1 4 3
conv N=2 H=64 W=76 Cin=640 Cout=256 KH=1 KW=1 stride=1 epi=0 korder=0 pool2=1 ln=0 shuffle2=0 tile=0 fp16=1 -> igemm 64 64 2 8 1 4 3
conv N=1 H=256 W=304 Cin=384 Cout=128 KH=1 KW=1 stride=1 epi=5 korder=0 pool2=0 ln=0 shuffle2=0 tile=20 fp16=0 -> igemm 64 64 2 8 1 4 2
conv N=1 H=256 W=304 Cin=384 Cout=128 KH=1 KW=1 stride=1 epi=5 korder=0 pool2=0 ln=0 shuffle2=0 tile=20 fp16=1 -> igemm 128 128 2 4 1 8 2
conv N=1 H=256 W=304 Cin=128 Cout=128 KH=1 KW=1 stride=1 epi=0 korder=0 pool2=0 ln=1 shuffle2=0 tile=0 fp16=1 -> igemm 128 128 2 4 1 8 1
conv N=1 H=64 W=76 Cin=256 Cout=32 KH=1 KW=1 stride=1 epi=0 korder=0 pool2=0 ln=1 shuffle2=0 tile=0 fp16=1 -> igemm 128 32 4 8 1 4 1
conv N=1 H=256 W=304 Cin=128 Cout=512 KH=1 KW=1 stride=1 epi=0 korder=0 pool2=0 ln=0 shuffle2=128 tile=0 fp16=1 -> igemm 128 128 2 4 1 8 0
conv N=1 H=256 W=304 Cin=64 Cout=64 KH=1 KW=1 stride=1 epi=0 korder=0 pool2=0 ln=0 shuffle2=0 tile=0 fp16=0 -> igemm 64 64 2 4 1 4 0
conv N=1 H=256 W=304 Cin=128 Cout=128 KH=3 KW=3 stride=2 epi=0 korder=0 pool2=0 ln=0 shuffle2=0 tile=12 fp16=1 -> E:conv2d: the halo tile needs a stride-1 kernel of at most 3x3 taps in K order 0
conv N=1 H=256 W=304 Cin=128 Cout=128 KH=3 KW=3 stride=1 epi=0 korder=0 pool2=0 ln=0 shuffle2=0 tile=14 fp16=1 -> E:conv2d: the pointwise kernel needs a 1x1 stride-1 layer
conv N=1 H=256 W=304 Cin=512 Cout=128 KH=1 KW=1 stride=1 epi=0 korder=0 pool2=0 ln=0 shuffle2=0 tile=14 fp16=0 -> E:conv2d: pointwise kernel: Cin=512 needs 316416 bytes of LDS
conv N=1 H=256 W=304 Cin=128 Cout=128 KH=3 KW=3 stride=1 epi=3 korder=2 pool2=0 ln=0 shuffle2=0 tile=4 fp16=1 -> E:conv2d: K order 2 with 128-pixel blocks takes one-operand epilogues only (epi=3 has two)
conv N=1 H=4 W=40 Cin=128 Cout=128 KH=3 KW=3 stride=1 epi=0 korder=2 pool2=0 ln=0 shuffle2=0 tile=40 fp16=1 -> frag 128 128 4 40 0
conv N=3 H=9 W=70 Cin=192 Cout=576 KH=3 KW=3 stride=1 epi=0 korder=2 pool2=0 ln=0 shuffle2=0 tile=40 fp16=1 -> frag 192 192 4 40 0
conv N=1 H=5 W=41 Cin=128 Cout=128 KH=3 KW=3 stride=1 epi=2 korder=2 pool2=0 ln=0 shuffle2=0 tile=40 fp16=1 -> frag 128 128 4 40 1
conv N=1 H=5 W=41 Cin=128 Cout=128 KH=3 KW=3 stride=1 epi=0 korder=2 pool2=0 ln=0 shuffle2=0 tile=4 fp16=1 -> frag 128 128 4 32 0
conv N=1 H=256 W=304 Cin=128 Cout=128 KH=3 KW=3 stride=1 epi=0 korder=2 pool2=0 ln=0 shuffle2=0 tile=2 fp16=1 -> frag 128 128 2 32 0
conv N=1 H=5 W=41 Cin=128 Cout=128 KH=3 KW=3 stride=1 epi=0 korder=2 pool2=0 ln=0 shuffle2=0 tile=0 fp16=1 -> frag 128 128 2 32 0
conv N=1 H=256 W=304 Cin=128 Cout=128 KH=3 KW=3 stride=1 epi=3 korder=2 pool2=0 ln=0 shuffle2=0 tile=40 fp16=1 -> E:conv2d: K order 2 with 160-pixel blocks takes one-operand epilogues only (epi=3 has two)
conv N=1 H=256 W=304 Cin=128 Cout=128 KH=1 KW=3 stride=1 epi=4 korder=2 pool2=0 ln=0 shuffle2=0 tile=40 fp16=1 -> E:conv2d: K order 2 with 160-pixel blocks takes one-operand epilogues only (epi=4 has two)
conv N=1 H=256 W=304 Cin=128 Cout=128 KH=1 KW=1 stride=1 epi=0 korder=0 pool2=0 ln=1 shuffle2=0 tile=7 fp16=1 -> E:conv2d: tile 7 has no pre-LayerNorm variant (2, 3, 6, 20 do)
conv N=1 H=256 W=304 Cin=128 Cout=128 KH=3 KW=3 stride=1 epi=0 korder=0 pool2=0 ln=0 shuffle2=0 tile=28 fp16=1 -> E:conv2d: unknown tile id 28
conv N=1 H=33 W=61 Cin=128 Cout=128 KH=3 KW=3 stride=2 epi=0 korder=0 pool2=0 ln=0 shuffle2=0 tile=0 fp16=1 -> igemm 64 64 2 8 1 4 0
conv N=2 H=1024 W=1216 Cin=16 Cout=64 KH=5 KW=5 stride=2 epi=0 korder=0 pool2=0 ln=0 shuffle2=0 tile=0 fp16=0 -> igemm 64 64 2 4 1 4 0
conv N=1 H=33 W=61 Cin=16 Cout=64 KH=5 KW=5 stride=2 epi=0 korder=0 pool2=0 ln=0 shuffle2=0 tile=0 fp16=0 -> igemm 64 64 2 4 1 4 0
conv N=2 H=256 W=304 Cin=32 Cout=128 KH=3 KW=3 stride=2 epi=0 korder=0 pool2=0 ln=0 shuffle2=0 tile=0 fp16=1 -> igemm 128 128 2 4 1 8 0
conv N=2 H=256 W=304 Cin=32 Cout=128 KH=3 KW=3 stride=2 epi=0 korder=0 pool2=0 ln=0 shuffle2=0 tile=0 fp16=0 -> igemm 128 128 2 4 1 8 0
conv N=2 H=256 W=296 Cin=32 Cout=128 KH=3 KW=3 stride=2 epi=0 korder=0 pool2=0 ln=0 shuffle2=0 tile=0 fp16=1 -> igemm 64 64 2 4 1 4 0
conv N=2 H=256 W=296 Cin=32 Cout=128 KH=3 KW=3 stride=2 epi=0 korder=0 pool2=0 ln=0 shuffle2=0 tile=0 fp16=0 -> igemm 64 64 2 4 1 4 0
conv N=1 H=33 W=61 Cin=32 Cout=64 KH=1 KW=1 stride=2 epi=0 korder=0 pool2=0 ln=0 shuffle2=0 tile=14 fp16=1 -> E:conv2d: the pointwise kernel needs a 1x1 stride-1 layer
chain C=128 dtype=1 rows=155648 nstage=2 nfan=0 weight_frag=1 xcd_group_rows=0 -> direct BM=64 NW=4 WP=0 xcd=0
chain C=128 dtype=1 rows=38912 nstage=0 nfan=1 weight_frag=1 xcd_group_rows=0 -> fan_only BM=64 NW=4 WP=0 xcd=0
chain C=128 dtype=1 rows=9728 nstage=0 nfan=2 weight_frag=1 xcd_group_rows=0 -> fan_only BM=32 NW=4 WP=0 xcd=0
chain C=256 dtype=1 rows=9728 nstage=2 nfan=0 weight_frag=1 xcd_group_rows=0 -> direct BM=64 NW=8 WP=0 xcd=0
chain C=256 dtype=1 rows=2432 nstage=1 nfan=3 weight_frag=1 xcd_group_rows=0 -> direct BM=32 NW=8 WP=0 xcd=0
chain C=256 dtype=1 rows=2432 nstage=3 nfan=3 weight_frag=1 xcd_group_rows=0 -> direct BM=32 NW=8 WP=0 xcd=0
chain C=256 dtype=1 rows=2432 nstage=3 nfan=1 weight_frag=1 xcd_group_rows=0 -> direct BM=32 NW=8 WP=0 xcd=0
chain C=128 dtype=1 rows=38912 nstage=1 nfan=0 weight_frag=1 xcd_group_rows=0 -> direct BM=64 NW=4 WP=0 xcd=0
chain C=256 dtype=1 rows=9728 nstage=0 nfan=3 weight_frag=1 xcd_group_rows=0 -> fan_only BM=64 NW=8 WP=0 xcd=0
chain C=256 dtype=1 rows=9728 nstage=3 nfan=3 weight_frag=1 xcd_group_rows=0 -> direct BM=64 NW=8 WP=0 xcd=0
chain C=256 dtype=1 rows=9728 nstage=3 nfan=0 weight_frag=1 xcd_group_rows=0 -> direct BM=64 NW=8 WP=0 xcd=0
chain C=256 dtype=1 rows=2432 nstage=0 nfan=1 weight_frag=1 xcd_group_rows=0 -> fan_only BM=32 NW=8 WP=0 xcd=0
chain C=256 dtype=1 rows=2432 nstage=0 nfan=3 weight_frag=1 xcd_group_rows=0 -> fan_only BM=32 NW=8 WP=0 xcd=0
chain C=128 dtype=1 rows=77824 nstage=1 nfan=0 weight_frag=1 xcd_group_rows=0 -> direct BM=64 NW=4 WP=0 xcd=0
chain C=128 dtype=1 rows=77824 nstage=2 nfan=0 weight_frag=1 xcd_group_rows=0 -> direct BM=64 NW=4 WP=0 xcd=0
chain C=128 dtype=1 rows=19456 nstage=0 nfan=1 weight_frag=1 xcd_group_rows=0 -> fan_only BM=32 NW=4 WP=0 xcd=0
chain C=128 dtype=1 rows=4864 nstage=0 nfan=1 weight_frag=1 xcd_group_rows=0 -> fan_only BM=32 NW=4 WP=0 xcd=0
chain C=128 dtype=1 rows=1216 nstage=1 nfan=3 weight_frag=1 xcd_group_rows=0 -> direct BM=32 NW=4 WP=0 xcd=0
chain C=128 dtype=1 rows=1216 nstage=3 nfan=3 weight_frag=1 xcd_group_rows=0 -> direct BM=32 NW=4 WP=0 xcd=0
chain C=128 dtype=1 rows=1216 nstage=3 nfan=1 weight_frag=1 xcd_group_rows=0 -> direct BM=32 NW=4 WP=0 xcd=0
chain C=128 dtype=1 rows=4864 nstage=1 nfan=0 weight_frag=1 xcd_group_rows=0 -> direct BM=32 NW=4 WP=0 xcd=0
chain C=128 dtype=1 rows=19456 nstage=1 nfan=0 weight_frag=1 xcd_group_rows=0 -> direct BM=32 NW=4 WP=0 xcd=0
chain C=128 dtype=1 rows=4864 nstage=0 nfan=2 weight_frag=1 xcd_group_rows=0 -> fan_only BM=32 NW=4 WP=0 xcd=0
chain C=256 dtype=1 rows=4864 nstage=2 nfan=0 weight_frag=1 xcd_group_rows=0 -> direct BM=32 NW=8 WP=0 xcd=0
chain C=256 dtype=1 rows=1216 nstage=1 nfan=3 weight_frag=1 xcd_group_rows=0 -> direct BM=32 NW=8 WP=0 xcd=0
chain C=256 dtype=1 rows=1216 nstage=3 nfan=3 weight_frag=1 xcd_group_rows=0 -> direct BM=32 NW=8 WP=0 xcd=0
chain C=256 dtype=1 rows=1216 nstage=3 nfan=1 weight_frag=1 xcd_group_rows=0 -> direct BM=32 NW=8 WP=0 xcd=0
chain C=192 dtype=1 rows=38912 nstage=2 nfan=0 weight_frag=1 xcd_group_rows=0 -> direct BM=64 NW=6 WP=0 xcd=0
chain C=192 dtype=1 rows=9728 nstage=3 nfan=3 weight_frag=1 xcd_group_rows=0 -> direct BM=32 NW=6 WP=0 xcd=0
chain C=192 dtype=1 rows=16385 nstage=1 nfan=0 weight_frag=1 xcd_group_rows=0 -> direct BM=64 NW=6 WP=0 xcd=0
chain C=128 dtype=1 rows=77824 nstage=3 nfan=0 weight_frag=1 xcd_group_rows=1216 -> direct BM=64 NW=4 WP=0 xcd=19
chain C=128 dtype=1 rows=9728 nstage=3 nfan=0 weight_frag=1 xcd_group_rows=1216 -> direct BM=32 NW=4 WP=0 xcd=38
chain C=128 dtype=1 rows=77824 nstage=3 nfan=0 weight_frag=1 xcd_group_rows=96 -> direct BM=64 NW=4 WP=0 xcd=0
chain C=256 dtype=1 rows=9728 nstage=2 nfan=0 weight_frag=0 xcd_group_rows=0 -> staged BM=64 NW=8 WP=4 xcd=0
chain C=256 dtype=1 rows=2432 nstage=2 nfan=0 weight_frag=0 xcd_group_rows=32 -> staged BM=32 NW=8 WP=4 xcd=0
chain C=128 dtype=0 rows=38912 nstage=3 nfan=0 weight_frag=0 xcd_group_rows=0 -> staged BM=32 NW=4 WP=4 xcd=0
chain C=512 dtype=1 rows=38912 nstage=2 nfan=0 weight_frag=1 xcd_group_rows=0 -> direct BM=32 NW=16 WP=0 xcd=0
chain C=384 dtype=1 rows=38912 nstage=2 nfan=0 weight_frag=0 xcd_group_rows=0 -> staged BM=32 NW=4 WP=4 xcd=0
chain C=256 dtype=1 rows=2048 nstage=2 nfan=0 weight_frag=0 xcd_group_rows=64 -> staged BM=32 NW=8 WP=4 xcd=2
"""

PROGRAM = r"""
#include <stdio.h>
#include <string.h>
#include "s2m2_amd/csrc/chain_select.h"
#include "s2m2_amd/csrc/conv_select.h"
struct Layer { int N, H, W, Ho, Wo, KH, KW, Cin, Cout, stride, epi, shuffle2, korder, pool2; const float* ln_wsum; };
int main() {
    static const char* family[] = {"error", "igemm", "igemm2", "halo", "frag", "pw"};
    static const int nparam[] = {0, 7, 4, 4, 5, 1};
    static const char* form[] = {"staged", "direct", "fan_only"};
    static const float wsum = 0.f;
    char line[512];
    while (fgets(line, sizeof line, stdin)) {
        line[strcspn(line, "\n")] = 0;
        Layer a{};
        int ln, tile, fp16, C, dtype, nstage, nfan, frag;
        long long rows, xcd;
        if (sscanf(line, "conv N=%d H=%d W=%d Cin=%d Cout=%d KH=%d KW=%d stride=%d epi=%d korder=%d pool2=%d ln=%d shuffle2=%d tile=%d fp16=%d", &a.N, &a.H, &a.W,
                   &a.Cin, &a.Cout, &a.KH, &a.KW, &a.stride, &a.epi, &a.korder, &a.pool2, &ln, &a.shuffle2, &tile, &fp16) == 15) {
            a.ln_wsum = ln ? &wsum : nullptr;
            a.Ho = (a.H + a.stride - 1) / a.stride; a.Wo = (a.W + a.stride - 1) / a.stride;
            if (a.pool2) { a.stride = 2; a.Ho = a.H / 2; a.Wo = a.W / 2; }                 // as conv2d_impl fills ConvArgs
            const s2m2::ConvChoice c = s2m2::conv_select(a, tile, fp16 != 0, s2m2::ConvTuning());
            printf("%s -> ", line);
            if (c.family == s2m2::ConvFamily::error) printf("E:%s", c.error);
            else {
                printf("%s", family[(int)c.family]);
                for (int i = 0; i < nparam[(int)c.family]; ++i) printf(" %d", c.p[i]);
            }
            printf("\n");
        } else if (sscanf(line, "chain C=%d dtype=%d rows=%lld nstage=%d nfan=%d weight_frag=%d xcd_group_rows=%lld", &C, &dtype, &rows, &nstage, &nfan, &frag, &xcd) == 7) {
            const s2m2::ChainChoice c = s2m2::chain_select(C, dtype, rows, nstage, nfan, frag, xcd, s2m2::ChainTuning());
            printf("%s -> %s BM=%d NW=%d WP=%d xcd=%d\n", line, form[(int)c.form], c.BM, c.NW, c.WP, c.xcd_tiles);
        }
    }
    return 0;
}
"""


def _compiler():
    for cc in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(cc)
        if path:
            return path
    raise RuntimeError("no host C++ compiler found (c++, g++, clang++)")


@pytest.fixture(scope="module")
def selected(tmp_path_factory):
    """descriptor -> choice, from one run of the host program over every descriptor of EXPECTED"""
    tmp = tmp_path_factory.mktemp("select")
    src, exe = tmp / "select.cpp", tmp / "select"
    src.write_text(PROGRAM)
    subprocess.run([_compiler(), "-std=c++17", "-O1", "-Wall", "-I", ROOT, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    wanted = [ln.split(" -> ")[0] for ln in EXPECTED.strip().splitlines()]
    out = subprocess.run([str(exe)], input="\n".join(wanted) + "\n", check=True, capture_output=True, text=True).stdout
    return dict(ln.split(" -> ", 1) for ln in out.strip().splitlines())


def test_headers_need_no_hip():
    """the two selectors include nothing from HIP (the compile in `selected` has no HIP include path either)"""
    for name in ("conv_select.h", "chain_select.h"):
        text = open(os.path.join(ROOT, "s2m2_amd", "csrc", name)).read()
        assert "hip/" not in text and "common.h" not in text, name


def test_selection_table(selected):
    expected = dict(ln.split(" -> ", 1) for ln in EXPECTED.strip().splitlines())
    assert len(expected) >= 80 and set(selected) == set(expected)
    wrong = [f"{k}\n    expected {v}\n    selected {selected[k]}" for k, v in expected.items() if selected[k] != v]
    assert not wrong, "\n".join(wrong)


def test_table_covers_every_family_and_form(selected):
    first = {v.split()[0].split(":")[0] for v in selected.values()}
    assert {"igemm", "halo", "frag", "E", "staged", "direct", "fan_only"} <= first
    assert any(v.startswith("frag 192 192") for v in selected.values())                    # the M model's 192-cout blocks
    assert any(v.startswith("igemm") and v.endswith(" 3") for v in selected.values())      # pool2
    assert any(v.startswith("igemm") and v.endswith(" 2") for v in selected.values())      # DUALMIX
    assert any(v.startswith("igemm") and v.endswith(" 1") for v in selected.values())      # pre-LayerNorm
