// The generic small step (step_small_grad.hip) with the layered MLT film (dchain.h ChainFilmLayers, "film_layers"): the same source, instantiated with the third film type in a unit of its own,
// so that the unit of the float and exact films holds no trace of it.
#define LMC_FILM_LAYERS_TU
#include "step_small_grad.hip"
