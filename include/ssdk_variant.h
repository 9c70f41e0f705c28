/*
 * ssdk_variant.h -- which template instance of a convolution kernel ran, part of libssdk.so (csrc/ssdk_api.cpp).
 *
 * A header of its own next to ssdk.h, like ssdk_dconv.h: the entry points of ssdk.h are a closed list under SSDK_VERSION 245, and this
 * addition changes neither them nor any descriptor.  Conventions (return values, thread-local text) are those of ssdk.h.
 *
 * ssdk_last_kernel() names the kernel the calling thread launched last; behind most names of ssdk_conv stand several template
 * instances and launcher branches (tile shapes, split-K, persistent or first form, layouts).  The launchers of ssdk_conv note the
 * instance as plain integers at the launch -- nothing is formatted on the launch path -- and this call makes the text on read:
 *
 *   "<instance> | <sizes>"      the part before " | " names the instance and the branch, the part behind it the numbers that change
 *                               with the layer's size (grid, patch, number of splits); kernels with no such numbers have no " | "
 *
 *   conv_gemm_kernel      gemm bn=<128|64|32|16> n64=<0|1> resv=<0|1> <split|unsplit> | splits=<n>
 *   conv_wave_kernel      wave <split|unsplit> | splits=<n>
 *   conv3x3_halo_kernel   halo <persistent|first> <nhwc|nchw> <split|unsplit>[ vec_nchw=<0|1>] | patch=<imgs>x<th>x<tw> ksplits=<n>
 *                         (vec_nchw: the first form with NCHW output only -- nothing else reads it)
 *   conv3x3_short_kernel  short cs=<1|2|3|4|8> <nhwc|nchw|nchw-wide> | nsplit=<n> tpw=<n>
 *   conv_smallmap_kernel  smallmap mfr=<4|8> taps=<1|9> packed=<0|1> na=<1|2> stride=<1|2> kw=<1|2> | cs=<4|8|16>
 *   pwflow_kernel         pwflow ks=<2|4|8> nf=<4|8|16> | slices=<n>
 *   conv_gemmp_kernel     gemmp <even|remainder> | grid=<n> tq=<n> tr=<n>
 *   conv_gemm256_kernel   gemm256 | tiles=<n>
 *   conv_first_kernel     first cout=<16|32|64> <nchw|nhwc>
 *   dwconv3x3_kernel      dw stride=<1|2>
 *
 * "" after a launch of any other kernel: the text always belongs to the kernel ssdk_last_kernel() names.  The pointer stays valid
 * until the calling thread asks again.  For tests and tools; nothing on the hot path reads it.
 */
#ifndef SSDK_VARIANT_H_
#define SSDK_VARIANT_H_

#ifdef __cplusplus
extern "C" {
#endif

const char* ssdk_last_variant(void);

#ifdef __cplusplus
}
#endif
#endif /* SSDK_VARIANT_H_ */
