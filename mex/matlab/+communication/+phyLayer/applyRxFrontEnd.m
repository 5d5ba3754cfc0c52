function rxWaveform = applyRxFrontEnd(rxWaveform, pathLoss, rxGain, noiseFigure, temperature, sampleRate)
%APPLYRXFRONTEND  The three lines that follow the channel in applyChannelModel (uePhy.m:748-754, gNBPhy.m:857-863) in one device pass:
%   db2mag(-pathLoss) * rx, .* 10^(rxGain/20), + sqrt(Nt/2) * complex(randn, randn) with Nt = k (T + 290 (F - 1)) fs.  rxWaveform is a MATLAB
%   array or a device handle (isac_mex('toDevice', ...) or the output of a handle-returning entry): a handle is modified in place and returned.
%   The noise is drawn HERE, by MATLAB's randn, in the reference's order (real part first), so the random stream of a simulation does not change.
    Nt = isac_mex('thermalNoisePower', double(temperature), double(noiseFigure), double(sampleRate));
    if isa(rxWaveform, 'uint64'), sz = isac_mex('size', rxWaveform); else, sz = size(rxWaveform); end
    rxWaveform = isac_mex('rxFrontEnd', rxWaveform, double(pathLoss), double(rxGain), Nt, complex(randn(sz), randn(sz)));
end
