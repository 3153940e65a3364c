/* TEST SCAFFOLDING, declarations only -- not FFTW, not a reference build.
 * tests/golden/make_fixtures.py compiles the reference's offt.h (from a reference checkout) to record the struct layouts
 * tests/test_boundary_pin.py compares ours with; that header needs the FFTW type and function NAMES it mentions to exist.
 * Nothing here is linked into the project or shipped. */
#ifndef OFFT_TEST_SHIM_FFTW3_H
#define OFFT_TEST_SHIM_FFTW3_H
typedef double fftw_complex[2];
typedef struct offt_test_shim_fftw_plan_s *fftw_plan;
#ifndef FFTW_MEASURE
#define FFTW_FORWARD (-1)
#define FFTW_BACKWARD (+1)
#define FFTW_MEASURE (0U)
#define FFTW_EXHAUSTIVE (1U << 3)
#define FFTW_PATIENT (1U << 5)
#define FFTW_ESTIMATE (1U << 6)
#endif
void fftw_execute(const fftw_plan p);
void fftw_destroy_plan(fftw_plan p);
void fftw_print_plan(const fftw_plan p);
void *fftw_malloc(unsigned long n);
void fftw_free(void *p);
#endif
