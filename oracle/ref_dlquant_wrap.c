/* TEST INFRASTRUCTURE: stand-ins and a flat entry point around the reference's own dlquant/quantizer.c, built by
 * build_ref_dlquant.sh into oracle/_ref/libdlquant_ref.so.  quantizer.c calls three mtPaint progress callbacks that
 * the reference does not define (and does not declare: the calls promote their arguments); they do nothing here and
 * never ask to stop. */
#include <stdint.h>
#include <stdlib.h>

#define REF_PALETTE_MAX 65536 /* quantizer.h PALETTE_MAX: userpal is uchar [3][PALETTE_MAX] */

int progress_init(char *text, int canc) {
    (void)text;
    (void)canc;
    return 0;
}

int progress_update(double val) {
    (void)val;
    return 0; /* 0: go on */
}

int progress_end(void) { return 0; }

int dl3quant(unsigned char *inbuf, int width, int height, int quant_to, int lookup_bpc,
             unsigned char userpal[3][REF_PALETTE_MAX]);

/* dl3quant over npix pixels (R, G, B bytes): pal[i] = r | g << 8 | b << 16 for the first quant_to entries of the
 * palette it returns, as or_dl3quant writes them.  Returns dl3quant's own result (0), or -1 without memory. */
int ref_dl3quant(const uint8_t *rgb, long npix, int quant_to, int bpc, int32_t *pal) {
    unsigned char(*up)[REF_PALETTE_MAX] = calloc(3, REF_PALETTE_MAX);
    if (!up) return -1;
    const int rc = dl3quant((unsigned char *)rgb, (int)npix, 1, quant_to, bpc, up);
    for (int i = 0; i < quant_to; i++) pal[i] = (int32_t)(up[0][i] | (up[1][i] << 8) | (up[2][i] << 16));
    free(up);
    return rc;
}
