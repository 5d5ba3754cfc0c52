function targets = targetList()
%TARGETLIST  Paired (range, velocity, azimuth) entries of the sensing.estimation.fft2D call made just before it.
%   fft2D's own rngEst / velEst / aziEst are three unrelated lists (fft2D.m:99 de-duplicates ranges and velocities
%   apart, aziEst comes from one covariance over the whole grid).  This joins them per detection on the MI355X: the
%   power window summed over the antennas, CFAR detections thinned to local maxima, a Bartlett azimuth of each
%   surviving cell's array snapshot on MUSIC's scan grid (ULA only).  Project-defined; no reference counterpart.
%   targets is an [n x 1] struct array, strongest first, with fields rng, vel, azi, power, hits, row, col.
%   Raises isac:INVALID_ARG when no completed fft2D precedes it, isac:UNSUPPORTED for a UPA.
    targets = isac_mex('fft2DTargets');
end
