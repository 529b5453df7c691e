/*
 * TEST INFRASTRUCTURE — not part of the product path.
 *
 * Prints the sizes and member offsets of struct coef, struct logger and struct progressbar in one line, as declared
 * by whichever headers the build selects:
 *   -DOUR_HEADERS                  include/jpeg2png_amd_compute.h         (tests/test_capi.py compiles this itself)
 *   -DREF_HEADERS                  the reference's jpeg2png.h, logger.h, progressbar.h, compute.h
 *   -DREF_HEADERS -DOUR_HEADERS    the reference's first, ours on top: the include guards must skip the re-definitions
 *                                  and the two compute() prototypes must be compatible
 * The two reference variants are built by oracle/Makefile (target ref-layout) into _ref/ where the reference sources
 * exist; what the reference's headers print is also kept in tests/golden/reference_struct_layouts.json.
 */
#include <stdio.h>
#include <stddef.h>
#ifdef REF_HEADERS
#include "jpeg2png.h"
#include "logger.h"
#include "progressbar.h"
#include "compute.h"
#endif
#ifdef OUR_HEADERS
#include "jpeg2png_amd_compute.h"
#endif

int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu %zu|", sizeof(struct coef), offsetof(struct coef, h), offsetof(struct coef, w),
           offsetof(struct coef, h_samp), offsetof(struct coef, w_samp), offsetof(struct coef, data),
           offsetof(struct coef, fdata), offsetof(struct coef, quant_table));
    printf("%zu %zu %zu %zu %zu|", sizeof(struct logger), offsetof(struct logger, f), offsetof(struct logger, filename),
           offsetof(struct logger, channel), offsetof(struct logger, iteration));
    printf("%zu %zu %zu\n", sizeof(struct progressbar), offsetof(struct progressbar, current), offsetof(struct progressbar, max));
    return 0;
}
