/* history_layout.c -- TEST HARNESS (tests/cpp, `make -f history.mk`; tests/test_history.py): struct sfl_history_record as a C
 * compiler sees it through include/sfl.h alone: its size, its offsets, and that its first 40 bytes are a struct sfl_flow_stats.
 * Prints them; exit status 0 = they are what the header states. */
#include <stddef.h>
#include <stdio.h>

#include "sfl.h"

int main(void)
{
    const size_t got[] = {sizeof(struct sfl_history_record),
                          offsetof(struct sfl_history_record, max_abs_vx), offsetof(struct sfl_history_record, max_abs_vy),
                          offsetof(struct sfl_history_record, max_abs_div), offsetof(struct sfl_history_record, what),
                          offsetof(struct sfl_history_record, dye_sum), offsetof(struct sfl_history_record, update_norm),
                          offsetof(struct sfl_history_record, iterations), offsetof(struct sfl_history_record, step),
                          offsetof(struct sfl_history_record, dt), offsetof(struct sfl_history_record, dx)};
    const size_t want[] = {64, 0, 4, 8, 12, 16, 40, 44, 48, 56, 60};
    int bad = 0;
    printf("sfl_history_record:");
    for (size_t k = 0; k < sizeof got / sizeof got[0]; ++k) {
        printf(" %zu", got[k]);
        bad += got[k] != want[k];
    }
    bad += offsetof(struct sfl_flow_stats, max_abs_div) != offsetof(struct sfl_history_record, max_abs_div);
    bad += offsetof(struct sfl_flow_stats, what) != offsetof(struct sfl_history_record, what);
    bad += offsetof(struct sfl_flow_stats, dye_sum) != offsetof(struct sfl_history_record, dye_sum);
    bad += sizeof(struct sfl_flow_stats) != offsetof(struct sfl_history_record, update_norm);
    printf("\n%d mismatches\n", bad);
    return bad != 0;
}
