// k_mala_finish (step_mala_phases.hip), the one splatting launch of the cache-filling pipeline, with the layered MLT film (dchain.h ChainFilmLayers, "film_layers"):
// the same source, instantiated with the third film type in a unit of its own.
#define LMC_FILM_LAYERS_TU
#include "step_mala_phases.hip"
