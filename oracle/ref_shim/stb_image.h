/* Declarations only: the three stb_image entry points the reference's bitmap texture calls.  oracle/ref_probe.cpp defines them
 * over the decoded pixels of its scene dump; the JPEG decode itself stays pinned by tests/golden/jpeg/. */
#pragma once
#ifdef __cplusplus
extern "C" {
#endif
unsigned char *stbi_load(char const *filename, int *x, int *y, int *channels_in_file, int desired_channels);
void stbi_image_free(void *retval_from_stbi_load);
const char *stbi_failure_reason(void);
#ifdef __cplusplus
}
#endif
